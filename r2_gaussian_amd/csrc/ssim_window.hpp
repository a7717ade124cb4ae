// ssim_window.hpp -- the SSIM window of r2_gaussian/utils/loss_utils.py:40-55 (11 taps, sigma 1.5, normalised in double, rounded
// to float once) and the 16 x 16 output tile with its 26 x 26 halo that the SSIM kernels stage in LDS (loss_ops.hip, metric_ops.hip).
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

}  // namespace r2
