// philox.hpp -- the project's counter-based generator: Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw: "Parallel random
// numbers: as easy as 1, 2, 3", SC 2011; the Random123 library), and the Box-Muller normals made of its words.  A value is a
// function of (seed, index, purpose, call) and of nothing else: no state, no order of evaluation, the same bits from any thread
// of any kernel and from the host.  Host-compilable, as gaussian_points.hpp's arithmetic is; tests/mcmc_ref.py restates it in
// numpy and holds the published known answers.
//
// The project's use (include/r2hip.h, "relocation and position noise"): key = the 64-bit seed (low word, high word); counter =
// (index, purpose, call low word, call high word); index = a row or a draw number; purpose = one of PHILOX_*.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define R2_PHILOX_HD __host__ __device__ __forceinline__
#else
#define R2_PHILOX_HD inline
#endif

namespace r2 {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;   // the two multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;   // the key increments (golden ratio, sqrt(3) - 1)
constexpr uint32_t PHILOX_NOISE = 0u, PHILOX_DRAW = 1u, PHILOX_SPREAD = 2u;   // the purposes

struct Philox4 {
    uint32_t w[4];
};

// ten rounds of  (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  the key bumped between rounds
R2_PHILOX_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Philox4{ { c0, c1, c2, c3 } };
}

R2_PHILOX_HD Philox4 philox_words(uint64_t seed, uint64_t call, uint32_t purpose, uint32_t index)
{
    return philox4x32_10(index, purpose, (uint32_t)call, (uint32_t)(call >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Box-Muller on two words: u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24 in [0, 1), both exact in float32;
// z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2), every operation a float32 one in the order written
R2_PHILOX_HD void philox_box_muller(uint32_t a, uint32_t b, float &z0, float &z1)
{
    const float u1 = (float)((a >> 8) + 1u) * 5.9604644775390625e-8f;
    const float u2 = (float)(b >> 8) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.0f * logf(u1));
    const float t = 6.283185307179586f * u2;
    z0 = r * cosf(t);
    z1 = r * sinf(t);
}

// the three normals of an index: z0, z1 of words (0, 1) and z0 of words (2, 3)
R2_PHILOX_HD void philox_normal3(uint64_t seed, uint64_t call, uint32_t purpose, uint32_t index, float e[3])
{
    const Philox4 p = philox_words(seed, call, purpose, index);
    float unused;
    philox_box_muller(p.w[0], p.w[1], e[0], e[1]);
    philox_box_muller(p.w[2], p.w[3], e[2], unused);
}

}  // namespace r2
