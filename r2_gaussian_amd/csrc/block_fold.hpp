// block_fold.hpp -- the fixed-order fold of one value per thread over a block of whole waves, which makes the sums of
// loss_ops.hip and metric_ops.hip bit-reproducible: xor-shuffles 32 down to 1 inside every wave, one LDS slot per wave, then
// thread 0 walks the slots 0, 1, 2, ... serially.  No atomics, the same order of combinations in every run.
#pragma once
#include "r2_common.hpp"

namespace r2 {

// a value of any type made of 32-bit words from lane (lane ^ d)
template <class T>
__device__ __forceinline__ T shfl_xor_words(T v, int d)
{
    static_assert(sizeof(T) % sizeof(int) == 0, "shuffled word by word");
    int w[sizeof(T) / sizeof(int)];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for (size_t i = 0; i < sizeof(T) / sizeof(int); ++i) w[i] = __shfl_xor(w[i], d);
    __builtin_memcpy(&v, w, sizeof(T));
    return v;
}

// op(a, b) combines two values (a is the thread's own or the running one).  slots: NW values in LDS; a block that folds
// through the same slots twice puts a __syncthreads() between the calls.  Every thread of the block calls this (it holds a
// barrier); the result is valid in thread 0 only.
template <int NW, class T, class Op>
__device__ __forceinline__ T block_fold(T v, T *slots, Op op)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, shfl_xor_words(v, d));
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = slots[0];
        for (int w = 1; w < NW; ++w) v = op(v, slots[w]);
    }
    return v;
}

// N sums that fold together, through one barrier
template <class T, int N>
struct Sums { T v[N]; };

struct FoldSum {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
    template <class T, int N>
    __device__ __forceinline__ Sums<T, N> operator()(Sums<T, N> a, Sums<T, N> b) const
    {
#pragma unroll
        for (int i = 0; i < N; ++i) a.v[i] += b.v[i];
        return a;
    }
};

}  // namespace r2
