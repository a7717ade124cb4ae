// median_select.hpp -- the forgetful selection of a median in registers, shared by the k x k median of projections.hip and the
// k-wide medians across detector columns of destripe.hip.  The median of n values is never the minimum or the maximum of any
// n / 2 + 2 of them: keep that many, find their minimum and maximum with min / max pairs, drop both, take one more value in,
// and end with three.  No value may be a NaN (the callers read a NaN as +inf).
#pragma once
#include <hip/hip_runtime.h>

namespace r2 {

__device__ __forceinline__ void order(float &a, float &b)
{
    const float lo = fminf(a, b);
    b = fmaxf(a, b);
    a = lo;
}

// the minimum of a[0 .. M-1] to a[0], the maximum to a[M-1]
template <int M>
__device__ __forceinline__ void min_max(float *a)
{
#pragma unroll
    for (int i = 0; i < M / 2; ++i) order(a[i], a[M - 1 - i]);
#pragma unroll
    for (int i = 1; i <= (M - 1) / 2; ++i) order(a[0], a[i]);
#pragma unroll
    for (int i = M / 2; i < M - 1; ++i) order(a[i], a[M - 1]);
}

// one round of the forgetful selection on M kept values, then the rounds below it; next(): the window's next value
template <int M, class Next>
__device__ __forceinline__ float select_median(float *a, Next next)
{
    min_max<M>(a);
    if constexpr (M == 3) {
        return a[1];
    } else {
        a[0] = next();   // a[M-1], the maximum, leaves by the shorter length
        return select_median<M - 1>(a, next);
    }
}

}  // namespace r2
