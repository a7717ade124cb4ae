// ssim_window.hpp -- the SSIM window of r2_gaussian/utils/loss_utils.py:40-55 (11 taps, sigma 1.5, normalised in double, rounded
// to float once) and the 16 x 16 output tile with its 26 x 26 halo that the SSIM kernels stage in LDS and blur in two passes
// (ssim_tile_moments: the forward pass of loss_ops.hip and the SSIM metric of metric_ops.hip, each through its own load).
#pragma once
#include "r2_common.hpp"
#include <math.h>

namespace r2 {

constexpr int SSIM_LT = 16;                      // output tile
constexpr int SSIM_WIN = 11, SSIM_HALO = SSIM_WIN / 2;
constexpr int SSIM_LR = SSIM_LT + 2 * SSIM_HALO; // staged region: 26 x 26

struct SsimWindow { float w[SSIM_WIN]; };

inline SsimWindow make_ssim_window()
{
    SsimWindow w;
    double g[SSIM_WIN], s = 0.0;
    for (int i = 0; i < SSIM_WIN; ++i) {
        g[i] = exp(-(double)((i - SSIM_HALO) * (i - SSIM_HALO)) / (2.0 * 1.5 * 1.5));
        s += g[i];
    }
    for (int i = 0; i < SSIM_WIN; ++i) w.w[i] = (float)(g[i] / s);
    return w;
}

// the LDS of one tile: the staged halo of both images (the centre of thread (tx, ty) is x[ty + SSIM_HALO][tx + SSIM_HALO],
// readable after ssim_tile_moments) and the horizontally blurred x, y, x^2, y^2, xy.  16-byte aligned arrays: y then lies a
// multiple of 256 bytes after x, and the x and y of one position move in one two-address LDS instruction
struct SsimTile {
    alignas(16) float x[SSIM_LR][SSIM_LR + 1];
    alignas(16) float y[SSIM_LR][SSIM_LR + 1];
    alignas(16) float hb[5][SSIM_LR][SSIM_LT + 1];
};

struct SsimMoments { float m1, m2, e11, e22, e12; };   // W*x, W*y, W*x^2, W*y^2, W*xy

// The tile (blockIdx.x, blockIdx.y) of a W x H image pair by a block of SSIM_LT^2 threads: stages the halo through
// load(gx, gy, inside) -> {x, y} (inside: the pixel lies in the image; what the loader returns outside is the padding), blurs
// the five moments horizontally then vertically and returns those of the thread's pixel (tid % SSIM_LT, tid / SSIM_LT).
template <class Load>
__device__ __forceinline__ SsimMoments ssim_tile_moments(SsimTile &t, int W, int H, const SsimWindow &win, Load load)
{
    constexpr int LT = SSIM_LT, LR = SSIM_LR;
    const int tid = threadIdx.x, tx = tid % LT, ty = tid / LT;
    const int ox = blockIdx.x * LT, oy = blockIdx.y * LT;
    for (int i = tid; i < LR * LR; i += LT * LT) {
        const int ry = i / LR, rx = i % LR, gx = ox + rx - SSIM_HALO, gy = oy + ry - SSIM_HALO;
        const float2 v = load(gx, gy, gx >= 0 && gx < W && gy >= 0 && gy < H);
        t.x[ry][rx] = v.x;
        t.y[ry][rx] = v.y;
    }
    __syncthreads();
    for (int i = tid; i < LR * LT; i += LT * LT) {
        const int ry = i / LT, cx = i % LT;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const float u = t.x[ry][cx + k], v = t.y[ry][cx + k], w = win.w[k];
            a += w * u; b += w * v; aa += w * (u * u); bb += w * (v * v); ab += w * (u * v);
        }
        t.hb[0][ry][cx] = a; t.hb[1][ry][cx] = b; t.hb[2][ry][cx] = aa; t.hb[3][ry][cx] = bb; t.hb[4][ry][cx] = ab;
    }
    __syncthreads();
    SsimMoments m = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < SSIM_WIN; ++k) {
        const float w = win.w[k];
        m.m1 += w * t.hb[0][ty + k][tx]; m.m2 += w * t.hb[1][ty + k][tx]; m.e11 += w * t.hb[2][ty + k][tx];
        m.e22 += w * t.hb[3][ty + k][tx]; m.e12 += w * t.hb[4][ty + k][tx];
    }
    return m;
}

}  // namespace r2
