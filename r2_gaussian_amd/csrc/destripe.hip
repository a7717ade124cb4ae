// destripe.hip -- stripe (ring-artefact) removal for measured projection stacks (projections.py: destripe, stripe_offsets): a
// detector pixel that is slightly off in every view is found by comparing neighbouring detector columns across all views.  The
// contract -- the stable order, the rank, the NaN rule, every float32 and double operation of the mean method -- is stated in
// include/r2hip.h (r2_proj_destripe_sort, r2_proj_destripe_mean); tests/destripe_ref.py restates it in NumPy / SciPy.
//
// The view axis of src[V][H][W] has a stride of H W floats, so the sort method works on the sinogram-major layout [H W][V], in
// which a pixel's column is contiguous, and meets the stack's own layout only in two tiled transposes:
//   1. transpose      src [V][HW] -> dst used as scratch [HW][V]: tiles of TR x TR = 64 x 64 through the LDS, so every view gives
//                     and every pixel takes a contiguous segment of 256 bytes.
//   2. sort_columns   a workgroup sorts SORT_ITEMS / N pixels' columns at once (one when N >= SORT_ITEMS = 512), N the power of
//                     two that holds V: 64-bit keys, (order-preserving bits of the float) << 32 | view, padded with maximal keys,
//                     in a bitonic network in the LDS -- the keys are distinct, so the stable order is the integer order and any
//                     network gives it.  The sorted values go back in place, the views to I (uint16) in the workspace.
//   3. median_putback a workgroup owns one detector row, MED_TW = 32 adjacent columns and MED_RC = 64 adjacent ranks.  It stages
//                     the MED_TW + k - 1 columns' rank segments (256 contiguous bytes each) in the LDS through clamped column
//                     indices; a lane owns one rank and 8 adjacent columns, selects each median in registers (the forgetful
//                     selection of median_select.hpp: k / 2 + 2 kept values, about 3 (k / 2 + 2)^2 / 4 min / max pairs -- 20 pairs
//                     for k = 9, 199 for k = 31 -- against the k^2 comparisons of rank counting) and puts it back at
//                     [pixel][I]: a scatter inside the pixel's own 4 V bytes of the workspace.
//   4. transpose      workspace [HW][V] -> dst [V][HW].
// The mean method is three passes: a lane per pixel walks the views with a double accumulator (lanes on adjacent pixels: every
// load is coalesced), a lane per pixel selects the median of the mean profile and writes the offset, and the subtraction.
// Every kernel walks its items with a grid-stride loop, so no launch depends on the stack's size.
#include "median_select.hpp"
#include "r2_common.hpp"
#include <math.h>
#include <type_traits>

namespace r2 {

namespace {

constexpr int TB = 256;                          // lanes of every workgroup here
constexpr int TR = 64;                           // transpose: side of a tile
constexpr int SORT_ITEMS = 512;                  // sort: keys of a workgroup when a column has fewer (two per lane)
constexpr int MED_TW = 32, MED_RC = 64;          // median: columns and ranks of a workgroup
constexpr int MED_COLS = MED_TW / (TB / MED_RC); // median: columns per lane
constexpr int SUB_VIEWS = 8;                     // mean: views per lane of the subtraction
constexpr unsigned GRID_CAP = 1u << 20;          // workgroups of a launch; the kernels loop beyond it

unsigned grid_for(size_t items) { return (unsigned)(items < GRID_CAP ? items : GRID_CAP); }

// in[R][C] -> out[C][R]
__global__ void __launch_bounds__(TB) destripe_transpose(size_t R, size_t C, const float *__restrict__ in, float *__restrict__ out)
{
    __shared__ float tile[TR][TR + 1];
    const size_t tiles_c = (C + TR - 1) / TR, tiles = ((R + TR - 1) / TR) * tiles_c;
    const int lx = (int)threadIdx.x % TR, ly = (int)threadIdx.x / TR;
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t r0 = t / tiles_c * TR, c0 = t % tiles_c * TR;
#pragma unroll
        for (int i = 0; i < TR; i += TB / TR)
            if (r0 + i + ly < R && c0 + lx < C) tile[i + ly][lx] = in[(r0 + i + ly) * C + c0 + lx];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TR; i += TB / TR)
            if (c0 + i + ly < C && r0 + lx < R) out[(c0 + i + ly) * R + r0 + lx] = tile[lx][i + ly];
        __syncthreads();
    }
}

// T[P][V]: the pixels' columns, sorted in place; I[P][V]: the view of every rank.  N = 1 << log_n >= V, G = max(1, SORT_ITEMS / N)
// columns per workgroup, keys[G * N] of dynamic LDS.
__global__ void __launch_bounds__(TB) destripe_sort_columns(size_t P, int V, int log_n, int G, float *__restrict__ T,
                                                            unsigned short *__restrict__ I)
{
    extern __shared__ unsigned long long keys[];
    const int N = 1 << log_n, items = G * N, tid = (int)threadIdx.x;
    const size_t groups = (P + G - 1) / G;
    for (size_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const size_t p0 = grp * G;
        const int cols = (int)(P - p0 < (size_t)G ? P - p0 : (size_t)G);
        for (int e = tid; e < items; e += TB) {
            const int g = e >> log_n, i = e & (N - 1);
            unsigned long long key = ~0ULL;
            if (g < cols && i < V) {
                float x = T[(p0 + g) * V + i];
                if (x != x) x = INFINITY;
                if (x == 0.0f) x = 0.0f;                                     // -0 orders as +0
                const unsigned u = __float_as_uint(x);
                key = (unsigned long long)(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u)) << 32 | (unsigned)i;
            }
            keys[e] = key;
        }
        __syncthreads();
        for (int k = 2; k <= N; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int c = tid; c < items / 2; c += TB) {
                    const int lo = ((c & ~(j - 1)) << 1) | (c & (j - 1)), hi = lo | j;
                    const bool ascending = (lo & k & (N - 1)) == 0;          // by the index inside the column; k = N: all ascending
                    const unsigned long long a = keys[lo], b = keys[hi];
                    if ((a > b) == ascending) {
                        keys[lo] = b;
                        keys[hi] = a;
                    }
                }
                __syncthreads();
            }
        for (int e = tid; e < items; e += TB) {
            const int g = e >> log_n, i = e & (N - 1);
            if (g < cols && i < V) {                                         // the padding sorts behind every real key
                const unsigned long long key = keys[e];
                const unsigned u = (unsigned)(key >> 32);
                T[(p0 + g) * V + i] = __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu));
                I[(p0 + g) * V + i] = (unsigned short)key;
            }
        }
        __syncthreads();
    }
}

// the median of the K values at(0) .. at(K-1), none of them a NaN
template <int K, class At>
__device__ __forceinline__ float median_of(At at)
{
    if constexpr (K == 1) {
        return at(0);
    } else {
        constexpr int KEEP = K / 2 + 2;
        float a[KEEP];
#pragma unroll
        for (int i = 0; i < KEEP; ++i) a[i] = at(i);
        int taken = KEEP;
        return select_median<KEEP>(a, [&]() { return at(taken++); });
    }
}

// S[H][W][V], the sorted sinogram; out[H][W][V]: out(h, w, I(h, w, r)) = median over the columns of S(h, clamp(w + j), r)
template <int K>
__global__ void __launch_bounds__(TB) destripe_median_putback(int H, int W, int V, const float *__restrict__ S,
                                                              const unsigned short *__restrict__ I, float *__restrict__ out)
{
    constexpr int R = K / 2, LW = MED_TW + 2 * R;
    __shared__ float tile[LW * MED_RC];
    const size_t strips = (size_t)(W + MED_TW - 1) / MED_TW, chunks = (size_t)(V + MED_RC - 1) / MED_RC;
    const size_t items = (size_t)H * strips * chunks;
    const int lr = (int)threadIdx.x % MED_RC, lc0 = (int)threadIdx.x / MED_RC * MED_COLS;
    for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int r0 = (int)(it % chunks) * MED_RC, w0 = (int)(it / chunks % strips) * MED_TW;
        const size_t row = it / (chunks * strips) * (size_t)W;              // the first pixel of detector row h
        for (int e = (int)threadIdx.x; e < LW * MED_RC; e += TB) {
            const int c = e / MED_RC, r = r0 + e % MED_RC;
            const int w = min(max(w0 + c - R, 0), W - 1);
            tile[e] = r < V ? S[(row + w) * V + r] : 0.0f;
        }
        __syncthreads();
        if (r0 + lr < V) {
#pragma unroll 1
            for (int u = 0; u < MED_COLS && w0 + lc0 + u < W; ++u) {
                const float *win = tile + (lc0 + u) * MED_RC + lr;          // column w + j - R of the window is win[j * MED_RC]
                const float m = median_of<K>([&](int j) { return win[j * MED_RC]; });
                const size_t o = (row + w0 + lc0 + u) * V;
                out[o + I[o + r0 + lr]] = m;
            }
        }
        __syncthreads();
    }
}

// the sort method with k = 1: out = in, a NaN as +inf
__global__ void __launch_bounds__(TB) destripe_copy(size_t n, const float *__restrict__ in, float *__restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * TB + threadIdx.x; i < n; i += (size_t)gridDim.x * TB) {
        const float x = in[i];
        out[i] = x != x ? INFINITY : x;
    }
}

// mean[P]: the pixels' means over the views, the sum in double in the views' order
__global__ void __launch_bounds__(TB) destripe_mean_profile(size_t P, int V, const float *__restrict__ src, float *__restrict__ mean)
{
    for (size_t p = (size_t)blockIdx.x * TB + threadIdx.x; p < P; p += (size_t)gridDim.x * TB) {
        double acc = 0.0;
#pragma unroll 8
        for (int v = 0; v < V; ++v) acc = acc + (double)src[(size_t)v * P + p];
        mean[p] = (float)(acc / (double)V);
    }
}

// d = mean - (median of the mean across the columns), to d[P] and, where given, to offsets[P]
template <int K>
__global__ void __launch_bounds__(TB) destripe_profile_offsets(size_t P, int W, const float *__restrict__ mean,
                                                               float *__restrict__ d, float *__restrict__ offsets)
{
    for (size_t p = (size_t)blockIdx.x * TB + threadIdx.x; p < P; p += (size_t)gridDim.x * TB) {
        const int w = (int)(p % (size_t)W);
        const float *row = mean + (p - w);
        const float s = median_of<K>([&](int j) {
            const float x = row[min(max(w + j - K / 2, 0), W - 1)];
            return x != x ? INFINITY : x;
        });
        const float off = mean[p] - s;
        d[p] = off;
        if (offsets) offsets[p] = off;
    }
}

// dst(v, p) = src(v, p) - d(p); the workgroups of one blockIdx.y share chunks of SUB_VIEWS views
__global__ void __launch_bounds__(TB) destripe_subtract(size_t P, int V, const float *__restrict__ src, const float *__restrict__ d,
                                                        float *__restrict__ dst)
{
    for (size_t p = (size_t)blockIdx.x * TB + threadIdx.x; p < P; p += (size_t)gridDim.x * TB) {
        const float off = d[p];
        for (long long v0 = (long long)blockIdx.y * SUB_VIEWS; v0 < V; v0 += (long long)gridDim.y * SUB_VIEWS) {
            const int v1 = (int)(v0 + SUB_VIEWS < V ? v0 + SUB_VIEWS : V);
#pragma unroll 4
            for (int v = (int)v0; v < v1; ++v) dst[(size_t)v * P + p] = src[(size_t)v * P + p] - off;
        }
    }
}

// f(std::integral_constant<int, k>) for the odd k in 1 .. 31
template <int K = 1, class F>
void with_width(int k, F f)
{
    if (k == K)
        f(std::integral_constant<int, K>{});
    else if constexpr (K < 31)
        with_width<K + 2>(k, f);
}

constexpr unsigned long long LIMIT_IMAGE = 0x80000000ULL, LIMIT_STACK = 1ULL << 38;

bool valid_stack(int V, int H, int W)
{
    return V >= 0 && H >= 1 && W >= 1 && (unsigned long long)H * W < LIMIT_IMAGE && (unsigned long long)V * H * W < LIMIT_STACK;
}

bool valid_width(int k) { return k >= 1 && k <= 31 && k % 2 == 1; }

}  // namespace

}  // namespace r2

extern "C" int r2_proj_destripe_max_views(void) { return R2_DESTRIPE_MAX_VIEWS; }

extern "C" size_t r2_proj_destripe_workspace_bytes(int V, int H, int W, int method)
{
    if (!r2::valid_stack(V, H, W)) return 0;
    const size_t P = (size_t)H * W;
    if (method == 0) return V <= R2_DESTRIPE_MAX_VIEWS ? P * V * (sizeof(float) + sizeof(unsigned short)) : 0;
    return method == 1 ? 2 * P * sizeof(float) : 0;
}

extern "C" int r2_proj_destripe_sort(int V, int H, int W, const float *src, int k, float *dst, void *ws, size_t ws_bytes,
                                     void *stream)
{
    using namespace r2;
    if (!valid_stack(V, H, W) || !valid_width(k) || V > R2_DESTRIPE_MAX_VIEWS) {
        set_error("r2_proj_destripe_sort: invalid argument (%d x %d x %d, k %d; at most %d views)", V, H, W, k, R2_DESTRIPE_MAX_VIEWS);
        return R2_ERR_INVALID;
    }
    if (V == 0) return 0;
    if (!src || !dst || !ws) {
        set_error("r2_proj_destripe_sort: NULL pointer");
        return R2_ERR_INVALID;
    }
    const size_t need = r2_proj_destripe_workspace_bytes(V, H, W, 0);
    if (ws_bytes < need) {
        set_error("r2_proj_destripe_sort: workspace of %zu bytes, %zu needed", ws_bytes, need);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t P = (size_t)H * W;
    if (k == 1) {   // every median is its own value: src with its NaNs as +inf, in one pass
        destripe_copy<<<dim3(grid_for((P * V + TB - 1) / TB)), dim3(TB), 0, s>>>(P * V, src, dst);
        R2_STAGE_CHECK(0, s, "stripe removal (sort, k = 1)");
        return 0;
    }
    float *filtered = (float *)ws;                                   // [P][V]
    unsigned short *views = (unsigned short *)(filtered + P * V);    // [P][V]
    int log_n = 0;
    while ((1 << log_n) < V) ++log_n;
    const int N = 1 << log_n, G = N >= SORT_ITEMS ? 1 : SORT_ITEMS / N;
    const size_t tiles_in = ((size_t)(V + TR - 1) / TR) * ((P + TR - 1) / TR);
    destripe_transpose<<<dim3(grid_for(tiles_in)), dim3(TB), 0, s>>>((size_t)V, P, src, dst);
    destripe_sort_columns<<<dim3(grid_for((P + G - 1) / G)), dim3(TB), (size_t)G * N * sizeof(unsigned long long), s>>>(P, V, log_n, G,
                                                                                                                      dst, views);
    const size_t items = (size_t)H * ((size_t)(W + MED_TW - 1) / MED_TW) * ((size_t)(V + MED_RC - 1) / MED_RC);
    with_width(k, [&](auto kc) {
        destripe_median_putback<decltype(kc)::value><<<dim3(grid_for(items)), dim3(TB), 0, s>>>(H, W, V, dst, views, filtered);
    });
    destripe_transpose<<<dim3(grid_for(tiles_in)), dim3(TB), 0, s>>>(P, (size_t)V, filtered, dst);
    R2_STAGE_CHECK(0, s, "stripe removal (sort)");
    return 0;
}

extern "C" int r2_proj_destripe_mean(int V, int H, int W, const float *src, int k, float *dst, float *offsets, void *ws,
                                     size_t ws_bytes, void *stream)
{
    using namespace r2;
    if (!valid_stack(V, H, W) || !valid_width(k)) {
        set_error("r2_proj_destripe_mean: invalid argument (%d x %d x %d, k %d)", V, H, W, k);
        return R2_ERR_INVALID;
    }
    if (V == 0) return 0;
    if (!src || (!dst && !offsets) || !ws) {
        set_error("r2_proj_destripe_mean: NULL pointer");
        return R2_ERR_INVALID;
    }
    const size_t need = r2_proj_destripe_workspace_bytes(V, H, W, 1);
    if (ws_bytes < need) {
        set_error("r2_proj_destripe_mean: workspace of %zu bytes, %zu needed", ws_bytes, need);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t P = (size_t)H * W;
    float *mean = (float *)ws, *d = mean + P;
    const unsigned blocks = grid_for((P + TB - 1) / TB);
    destripe_mean_profile<<<dim3(blocks), dim3(TB), 0, s>>>(P, V, src, mean);
    with_width(k, [&](auto kc) {
        destripe_profile_offsets<decltype(kc)::value><<<dim3(blocks), dim3(TB), 0, s>>>(P, W, mean, d, offsets);
    });
    if (dst) {
        // enough workgroups to fill the chip when the detector alone does not: at most 65535 along y, 2^16 + 2^20 in all
        const unsigned chunks = (unsigned)(((long long)V + SUB_VIEWS - 1) / SUB_VIEWS), share = 65535u / blocks;
        destripe_subtract<<<dim3(blocks, chunks < share ? chunks : (share ? share : 1u)), dim3(TB), 0, s>>>(P, V, src, d, dst);
    }
    R2_STAGE_CHECK(0, s, "stripe removal (mean)");
    return 0;
}
