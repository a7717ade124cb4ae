// spline.hip -- cubic B-spline resampling of volumes (resample.py: spline_filter, zoom, map_coordinates): the prefilter that
// turns samples into B-spline coefficients, and the two evaluators of the spline, on a regular output grid (zoom) and at
// arbitrary points (sample).  Together they are scipy.ndimage's zoom / map_coordinates for order 3 and mode "nearest".  The
// contract -- the padding, the recursion, the start values, the weight formulas and the order of every operation -- is stated
// in include/r2hip.h (r2_spline_prefilter, r2_spline_zoom, r2_spline_sample); tests/resample_ref.py restates it in float32
// operation for operation, which is why this file is compiled without FMA contraction.
//
// The prefilter is a recursive filter along every line of the padded block, along x, then y, then z.  A line is serial, so the
// parallelism is across lines.  Along x and y a lane owns a line and neighbouring lanes own neighbouring z, so that every step
// of the recursion is one coalesced row (spline_filter_x, spline_filter_y); the x pass reads the unpadded input through
// clamped indices, so the padded copy is never made.  Along z the lines themselves are the contiguous direction: a one-wave
// workgroup takes ZT_LINES lines, moves ZT_CHUNK of their elements at a time through an LDS tile (rows loaded and stored
// coalesced, the recursion run by one lane per line down its own row of the tile, stride ZT_STRIDE against bank conflicts),
// and carries the recursion's state in a register from chunk to chunk: forwards for the causal sweep, backwards for the
// anti-causal one.
#include "r2_common.hpp"
#include <math.h>

namespace r2 {

namespace {

constexpr int PAD = R2_SPLINE_PAD;
constexpr int HORIZON = R2_SPLINE_HORIZON;
constexpr int TB = 256;                                        // x / y passes, zoom, sample: threads per workgroup
constexpr int BATCH = 8;                                       // x / y passes: loads in flight per lane
constexpr int ZT_LINES = 64, ZT_CHUNK = 64, ZT_STRIDE = 65;    // z pass: lines per workgroup, elements per chunk, LDS row stride
constexpr int ZT_BATCH = 16;                                   // z pass: rows of a tile in flight per lane

// the pole of the cubic B-spline, the gain and the powers of the pole: computed in double, rounded once
struct Filter {
    float z, gain, anti;
    float zp[HORIZON + 1];
};

Filter make_filter()
{
    const double z = sqrt(3.0) - 2.0;
    Filter f;
    f.z = (float)z;
    f.gain = (float)((1.0 - z) * (1.0 - 1.0 / z));
    f.anti = (float)(z / (z - 1.0));
    f.zp[0] = 1.0f;
    for (int i = 1; i <= HORIZON; ++i) f.zp[i] = (float)pow(z, (double)i);
    return f;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The line filter of r2hip.h on a strided line of n elements in memory: in(i) is the line's input (before the gain), dst its
// place in the coefficients.  The causal sweep writes dst, the anti-causal one reads it back and overwrites it.
template <class In>
__device__ __forceinline__ void filter_line(const Filter &f, int n, In in, float *dst, size_t stride)
{
    const float g0 = f.gain * in(0);
    float s = g0;
#pragma unroll
    for (int i = 1; i <= HORIZON; ++i) s = s + f.zp[i] * (f.gain * in(i));
    float c = g0 + f.z * s;
    dst[0] = c;
    // BATCH loads are issued before the steps that consume them: a line's loads do not depend on its recursion
    int i = 1;
    for (; i + BATCH <= n; i += BATCH) {
        float v[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) v[u] = in(i + u);
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            c = f.gain * v[u] + f.z * c;
            dst[(size_t)(i + u) * stride] = c;
        }
    }
    for (; i < n; ++i) {
        c = f.gain * in(i) + f.z * c;
        dst[(size_t)i * stride] = c;
    }
    c = c * f.anti;
    dst[(size_t)(n - 1) * stride] = c;
    i = n - 2;
    for (; i - BATCH + 1 >= 0; i -= BATCH) {
        float v[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) v[u] = dst[(size_t)(i - u) * stride];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            c = f.z * (c - v[u]);
            dst[(size_t)(i - u) * stride] = c;
        }
    }
    for (; i >= 0; --i) {
        c = f.z * (c - dst[(size_t)i * stride]);
        dst[(size_t)i * stride] = c;
    }
}

// x pass: one lane per (j, k) of the padded block, reading the unpadded volume at clamped indices
__global__ void __launch_bounds__(TB) spline_filter_x(Filter f, int nx, int ny, int nz, const float *__restrict__ vol,
                                                      float *__restrict__ coeffs)
{
    const int nyp = ny + 2 * PAD, nzp = nz + 2 * PAD;
    const size_t plane = (size_t)nyp * nzp;
    const size_t q = (size_t)blockIdx.x * TB + threadIdx.x;
    if (q >= plane) return;
    const int j = (int)(q / (size_t)nzp), k = (int)(q % (size_t)nzp);
    const size_t vplane = (size_t)ny * nz;
    const float *src = vol + (size_t)clampi(j - PAD, 0, ny - 1) * nz + (size_t)clampi(k - PAD, 0, nz - 1);
    filter_line(f, nx + 2 * PAD, [&](int i) { return src[(size_t)clampi(i - PAD, 0, nx - 1) * vplane]; }, coeffs + q, plane);
}

// y pass, in place: one lane per (i, k)
__global__ void __launch_bounds__(TB) spline_filter_y(Filter f, int nxp, int nyp, int nzp, float *coeffs)
{
    const size_t q = (size_t)blockIdx.x * TB + threadIdx.x;
    if (q >= (size_t)nxp * nzp) return;
    const int i = (int)(q / (size_t)nzp), k = (int)(q % (size_t)nzp);
    float *line = coeffs + (size_t)i * nyp * nzp + k;
    filter_line(f, nyp, [&](int j) { return line[(size_t)j * nzp]; }, line, (size_t)nzp);
}

// z pass: ZT_BATCH rows of the tile between memory and LDS with their loads (LDS reads) issued together.  LOAD: memory ->
// tile, times `scale`; otherwise tile -> memory.  Rows beyond nrows are read at the last row and dropped.
template <bool LOAD>
__device__ __forceinline__ void tile_rows(float *tile, float *base, int nrows, int nzp, int k0, int len, int lane, float scale)
{
    if (lane >= len) return;
    for (int r0 = 0; r0 < nrows; r0 += ZT_BATCH) {
        float v[ZT_BATCH];
#pragma unroll
        for (int u = 0; u < ZT_BATCH; ++u) {
            const int r = min(r0 + u, nrows - 1);
            v[u] = LOAD ? base[(size_t)r * nzp + k0 + lane] : tile[r * ZT_STRIDE + lane];
        }
#pragma unroll
        for (int u = 0; u < ZT_BATCH; ++u) {
            const int r = r0 + u;
            if (r < nrows) {
                if (LOAD) tile[r * ZT_STRIDE + lane] = scale * v[u];
                else base[(size_t)r * nzp + k0 + lane] = v[u];
            }
        }
    }
}

// z pass, in place: a wave per ZT_LINES lines, ZT_CHUNK elements at a time through LDS.  A lane walks its own row of the tile
// BATCH elements at a time, read together before the steps that consume them.
__global__ void __launch_bounds__(ZT_LINES) spline_filter_z(Filter f, long long rows, int nzp, float *coeffs)
{
    __shared__ float tile[ZT_LINES * ZT_STRIDE];
    const int lane = (int)threadIdx.x;
    const long long row0 = (long long)blockIdx.x * ZT_LINES;
    const int nrows = (int)min((long long)ZT_LINES, rows - row0);
    float *base = coeffs + (size_t)row0 * nzp;
    float *mine = tile + lane * ZT_STRIDE;
    const int nch = (nzp + ZT_CHUNK - 1) / ZT_CHUNK;
    float c = 0.0f;
    for (int ch = 0; ch < nch; ++ch) {
        const int k0 = ch * ZT_CHUNK, len = min(ZT_CHUNK, nzp - k0);
        tile_rows<true>(tile, base, nrows, nzp, k0, len, lane, f.gain);
        __syncthreads();
        if (lane < nrows) {
            int k = 0;
            if (ch == 0) {   // the first chunk holds at least 2 PAD + 1 > HORIZON elements
                float s = mine[0];
#pragma unroll
                for (int i = 1; i <= HORIZON; ++i) s = s + f.zp[i] * mine[i];
                c = mine[0] + f.z * s;
                mine[0] = c;
                k = 1;
            }
            for (; k + BATCH <= len; k += BATCH) {
                float v[BATCH];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) v[u] = mine[k + u];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    c = v[u] + f.z * c;
                    mine[k + u] = c;
                }
            }
            for (; k < len; ++k) {
                c = mine[k] + f.z * c;
                mine[k] = c;
            }
        }
        __syncthreads();
        tile_rows<false>(tile, base, nrows, nzp, k0, len, lane, 1.0f);
        __syncthreads();
    }
    for (int ch = nch - 1; ch >= 0; --ch) {
        const int k0 = ch * ZT_CHUNK, len = min(ZT_CHUNK, nzp - k0);
        tile_rows<true>(tile, base, nrows, nzp, k0, len, lane, 1.0f);
        __syncthreads();
        if (lane < nrows) {
            int k = len - 1;
            if (ch == nch - 1) {
                c = mine[k] * f.anti;
                mine[k] = c;
                --k;
            }
            for (; k - BATCH + 1 >= 0; k -= BATCH) {
                float v[BATCH];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) v[u] = mine[k - u];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    c = f.z * (c - v[u]);
                    mine[k - u] = c;
                }
            }
            for (; k >= 0; --k) {
                c = f.z * (c - mine[k]);
                mine[k] = c;
            }
        }
        __syncthreads();
        tile_rows<false>(tile, base, nrows, nzp, k0, len, lane, 1.0f);
        __syncthreads();
    }
}

// the four weights of the fraction t, in T's precision and r2hip.h's order
template <class T>
__device__ __forceinline__ void bspline_weights(T t, T w[4])
{
    const T one = (T)1, two = (T)2, three = (T)3, four = (T)4, six = (T)6;
    w[1] = (t * t * (t - two) * three + four) / six;
    const T u = one - t;
    w[2] = (u * u * (u - two) * three + four) / six;
    w[0] = u * u * u / six;
    w[3] = one - w[0] - w[1] - w[2];
}

// The zoom's tables in the workspace: int start[M], then float w[4][M], M = mx + my + mz, the axes one after the other.
struct Tables {
    const int *start;
    const float *w;
    int M;
};

__global__ void __launch_bounds__(TB) spline_zoom_tables(int mx, int my, int mz, double fx, double fy, double fz, int *start,
                                                         float *w)
{
    const int M = mx + my + mz;
    const int e = (int)(blockIdx.x * TB + threadIdx.x);
    if (e >= M) return;
    const int o = e < mx ? e : (e < mx + my ? e - mx : e - mx - my);
    const double f = e < mx ? fx : (e < mx + my ? fy : fz);
    const double cc = (double)o * f + (double)PAD;
    const double fl = floor(cc);
    double wd[4];
    bspline_weights<double>(cc - fl, wd);
    start[e] = (int)fl - 1;
    for (int k = 0; k < 4; ++k) w[(size_t)k * M + e] = (float)wd[k];
}

// sum_i wx_i (sum_j wy_j (sum_k wz_k c(sx + i, sy + j, sz + k))), each sum left to right
__device__ __forceinline__ float spline_taps(const float *__restrict__ c, size_t stride_x, size_t stride_y, const int ix[4],
                                             const int iy[4], const int iz[4], const float wx[4], const float wy[4],
                                             const float wz[4])
{
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float inner = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float *p = c + (size_t)ix[i] * stride_x + (size_t)iy[j] * stride_y;
            float line = wz[0] * p[iz[0]];
            line = line + wz[1] * p[iz[1]];
            line = line + wz[2] * p[iz[2]];
            line = line + wz[3] * p[iz[3]];
            inner = j == 0 ? wy[0] * line : inner + wy[j] * line;
        }
        acc = i == 0 ? wx[0] * inner : acc + wx[i] * inner;
    }
    return acc;
}

// one lane per output voxel, neighbouring lanes on neighbouring output z
__global__ void __launch_bounds__(TB) spline_zoom(int nyp, int nzp, const float *__restrict__ coeffs, int mx, int my, int mz,
                                                  Tables t, float *__restrict__ out)
{
    const size_t o = (size_t)blockIdx.x * TB + threadIdx.x;
    if (o >= (size_t)mx * my * mz) return;
    const int e[3] = {(int)(o / ((size_t)my * mz)), mx + (int)((o / (size_t)mz) % (size_t)my), mx + my + (int)(o % (size_t)mz)};
    int idx[3][4];
    float w[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            idx[a][k] = t.start[e[a]] + k;
            w[a][k] = t.w[(size_t)k * t.M + e[a]];
        }
    out[o] = spline_taps(coeffs, (size_t)nyp * nzp, (size_t)nzp, idx[0], idx[1], idx[2], w[0], w[1], w[2]);
}

// one lane per point
__global__ void __launch_bounds__(TB) spline_sample(int nxp, int nyp, int nzp, const float *__restrict__ coeffs, int N,
                                                    const float *__restrict__ points, float *__restrict__ out)
{
    const int p = (int)(blockIdx.x * TB + threadIdx.x);
    if (p >= N) return;
    const float x[3] = {points[3 * (size_t)p], points[3 * (size_t)p + 1], points[3 * (size_t)p + 2]};
    if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) {
        out[p] = NAN;
        return;
    }
    const int np[3] = {nxp, nyp, nzp};
    int idx[3][4];
    float w[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float cc = x[a] + (float)PAD;
        cc = fminf(fmaxf(cc, -1.0f), (float)np[a]);
        const float fl = floorf(cc);
        bspline_weights<float>(cc - fl, w[a]);
        const int start = (int)fl - 1;
#pragma unroll
        for (int k = 0; k < 4; ++k) idx[a][k] = clampi(start + k, 0, np[a] - 1);
    }
    out[p] = spline_taps(coeffs, (size_t)nyp * nzp, (size_t)nzp, idx[0], idx[1], idx[2], w[0], w[1], w[2]);
}

// the padded element count, or 0 for dimensions the entries refuse
size_t padded_count(int nx, int ny, int nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    const unsigned long long a = (unsigned long long)nx + 2 * PAD, b = (unsigned long long)ny + 2 * PAD,
                             c = (unsigned long long)nz + 2 * PAD;
    if (a * b >= 0x80000000ULL || a * b * c >= 0x80000000ULL) return 0;
    return (size_t)(a * b * c);
}

unsigned blocks_for(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

}  // namespace r2

extern "C" int r2_spline_prefilter_pass(int nx, int ny, int nz, const float *vol, float *coeffs, int axis, void *stream)
{
    using namespace r2;
    if (!padded_count(nx, ny, nz) || !coeffs || axis < 0 || axis > 2 || (axis == 0 && !vol)) {
        set_error("r2_spline_prefilter_pass: invalid argument (dimensions %d x %d x %d, axis %d)", nx, ny, nz, axis);
        return R2_ERR_INVALID;
    }
    const Filter f = make_filter();
    const int nxp = nx + 2 * PAD, nyp = ny + 2 * PAD, nzp = nz + 2 * PAD;
    hipStream_t s = (hipStream_t)stream;
    if (axis == 0)
        spline_filter_x<<<dim3(blocks_for((size_t)nyp * nzp, TB)), dim3(TB), 0, s>>>(f, nx, ny, nz, vol, coeffs);
    else if (axis == 1)
        spline_filter_y<<<dim3(blocks_for((size_t)nxp * nzp, TB)), dim3(TB), 0, s>>>(f, nxp, nyp, nzp, coeffs);
    else
        spline_filter_z<<<dim3(blocks_for((size_t)nxp * nyp, ZT_LINES)), dim3(ZT_LINES), 0, s>>>(f, (long long)nxp * nyp, nzp,
                                                                                                  coeffs);
    R2_STAGE_CHECK(0, s, "spline prefilter");
    return 0;
}

extern "C" int r2_spline_prefilter(int nx, int ny, int nz, const float *vol, float *coeffs, void *stream)
{
    if (!r2::padded_count(nx, ny, nz) || !vol || !coeffs) {
        r2::set_error("r2_spline_prefilter: invalid argument (dimensions %d x %d x %d)", nx, ny, nz);
        return R2_ERR_INVALID;
    }
    for (int axis = 0; axis < 3; ++axis) {
        const int rc = r2_spline_prefilter_pass(nx, ny, nz, vol, coeffs, axis, stream);
        if (rc < 0) return rc;
    }
    return 0;
}

extern "C" size_t r2_spline_zoom_workspace_bytes(int mx, int my, int mz)
{
    if (mx < 1 || my < 1 || mz < 1) return 0;
    return ((size_t)mx + my + mz) * (sizeof(int) + 4 * sizeof(float));
}

extern "C" int r2_spline_zoom(int nx, int ny, int nz, const float *coeffs, int mx, int my, int mz, float *out, void *ws,
                              size_t ws_bytes, void *stream)
{
    using namespace r2;
    const unsigned long long mtot = mx < 1 || my < 1 || mz < 1 ? 0 : (unsigned long long)mx * my * mz;
    if (!padded_count(nx, ny, nz) || mtot == 0 || (unsigned long long)mx * my >= 0x80000000ULL || mtot >= 0x80000000ULL ||
        (unsigned long long)mx + my + mz >= 0x80000000ULL || !coeffs || !out || !ws) {
        set_error("r2_spline_zoom: invalid argument (%d x %d x %d -> %d x %d x %d)", nx, ny, nz, mx, my, mz);
        return R2_ERR_INVALID;
    }
    if (ws_bytes < r2_spline_zoom_workspace_bytes(mx, my, mz)) {
        set_error("r2_spline_zoom: workspace of %zu bytes, %zu needed", ws_bytes, r2_spline_zoom_workspace_bytes(mx, my, mz));
        return R2_ERR_INVALID;
    }
    const int M = mx + my + mz;
    int *start = (int *)ws;
    float *w = (float *)ws + M;
    const double fx = mx > 1 ? (double)(nx - 1) / (double)(mx - 1) : 1.0, fy = my > 1 ? (double)(ny - 1) / (double)(my - 1) : 1.0,
                 fz = mz > 1 ? (double)(nz - 1) / (double)(mz - 1) : 1.0;
    hipStream_t s = (hipStream_t)stream;
    spline_zoom_tables<<<dim3(blocks_for((size_t)M, TB)), dim3(TB), 0, s>>>(mx, my, mz, fx, fy, fz, start, w);
    spline_zoom<<<dim3(blocks_for((size_t)mtot, TB)), dim3(TB), 0, s>>>(ny + 2 * PAD, nz + 2 * PAD, coeffs, mx, my, mz,
                                                                        Tables{start, w, M}, out);
    R2_STAGE_CHECK(0, s, "spline zoom");
    return 0;
}

extern "C" int r2_spline_sample(int nx, int ny, int nz, const float *coeffs, int N, const float *points, float *out, void *stream)
{
    using namespace r2;
    if (!padded_count(nx, ny, nz) || N < 0 || !coeffs || (N > 0 && (!points || !out))) {
        set_error("r2_spline_sample: invalid argument (dimensions %d x %d x %d, N %d)", nx, ny, nz, N);
        return R2_ERR_INVALID;
    }
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    spline_sample<<<dim3(blocks_for((size_t)N, TB)), dim3(TB), 0, s>>>(nx + 2 * PAD, ny + 2 * PAD, nz + 2 * PAD, coeffs, N, points,
                                                                       out);
    R2_STAGE_CHECK(0, s, "spline sample");
    return 0;
}
