// graph_loss.hip -- the transposed neighbour graph (r2_graph_transpose) and a smoothness loss over the directed edges of a graph
// with its gradient (r2_graph_loss, r2_graph_loss_backward); contract in include/r2hip.h.  No counterpart in the reference.
//
// The loss sends gradient to both ends of an edge i -> j.  The i end is the node's own row; the j end needs the edges that point
// AT a node, in a fixed order, and that is what the transpose provides: a stable sort of the edge ids by target (radix_sort.hip),
// so the incoming edges of a node are in ascending edge id.  Every gradient is then one thread's (or one wave's) sum in a fixed
// order: no atomics, the same bits on every call.  Compiled with -ffp-contract=off: the per-term operation order below is the
// one the header states and tests/graph_ref.py bounds.
#include "r2_common.hpp"

#include <algorithm>
#include <cmath>

namespace r2 {
namespace {

constexpr int GL_THREADS = 256;
constexpr int GL_PER_THREAD = 8;                              // edges per thread of the forward (header: R2_GRAPH_LOSS_CHAIN)
constexpr int GL_BLOCK_EDGES = GL_THREADS * GL_PER_THREAD;
constexpr int GL_HUB = R2_GRAPH_LOSS_HUB;                     // longer incoming lists are summed by the whole wave
static_assert(GL_PER_THREAD + 6 + 2 + 1 == R2_GRAPH_LOSS_CHAIN, "the header states the forward's longest chain of additions");

// ---- transpose
__global__ void __launch_bounds__(256) graph_keys_kernel(int P, uint32_t n, const int *__restrict__ idx, uint32_t *__restrict__ keys)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= n) return;
    const int t = idx[e];
    keys[e] = (t >= 0 && t < P) ? (uint32_t)t : (uint32_t)P;   // invalid edges sort behind every node
}

// in_offsets[j] = number of sorted keys < j, j in [0, P]: the sorted keys are the targets, so this is where node j's list starts,
// and in_offsets[P] the number of valid edges
__global__ void __launch_bounds__(256) graph_offsets_kernel(int P, uint32_t n, const uint32_t *__restrict__ sorted_keys,
                                                            int *__restrict__ in_offsets)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j > (uint32_t)P) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sorted_keys[mid] < j) lo = mid + 1; else hi = mid;
    }
    in_offsets[j] = (int)lo;
}

// ---- the edge function.  a = value at the edge's source, b = value at its target, x = a - b (one rounding).
template <int KIND>
__device__ __forceinline__ float gl_phi(float a, float b, float delta)
{
    const float x = a - b;
    if (KIND == R2_GRAPH_KIND_L1) return fabsf(x);
    if (KIND == R2_GRAPH_KIND_L2) return x * x;
    const float ax = fabsf(x);
    return ax <= delta ? 0.5f * (x * x) : delta * (ax - 0.5f * delta);
}

template <int KIND>
__device__ __forceinline__ float gl_dphi(float a, float b, float delta)
{
    // kind 0 takes the sign from the comparison: tied values give exactly 0
    if (KIND == R2_GRAPH_KIND_L1) return a > b ? 1.0f : (a < b ? -1.0f : 0.0f);
    const float x = a - b;
    if (KIND == R2_GRAPH_KIND_L2) return 2.0f * x;
    return fabsf(x) <= delta ? x : copysignf(delta, x);
}

// ---- forward.  Workgroup b owns edges [2048 b, 2048 (b + 1)); thread t adds its 8 terms e = 2048 b + 256 k + t in ascending k
// (invalid edges and edges past the end add +0), the wave folds by xor butterfly (offsets 32, 16, .. 1), the four wave sums are
// combined as (s0 + s1) + (s2 + s3): 8 + 6 + 2 float additions on the longest chain.
template <int KIND, bool HAS_W>
__global__ void __launch_bounds__(GL_THREADS) graph_loss_fwd_kernel(int P, int K, uint32_t n, const float *__restrict__ v,
                                                                    const int *__restrict__ idx, const float *__restrict__ w,
                                                                    float delta, float *__restrict__ partial)
{
    __shared__ float red[GL_THREADS / 64];
    float acc = 0.0f;
    const uint32_t base = blockIdx.x * (uint32_t)GL_BLOCK_EDGES + threadIdx.x;
#pragma unroll
    for (int k = 0; k < GL_PER_THREAD; ++k) {
        const uint32_t e = base + (uint32_t)k * GL_THREADS;
        float t = 0.0f;
        if (e < n) {
            const int j = idx[e];
            if (j >= 0 && j < P) {
                t = gl_phi<KIND>(v[e / (uint32_t)K], v[j], delta);
                if (HAS_W) t = w[e] * t;
            }
        }
        acc += t;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the workgroups' partials in double, thread t taking t, t + 256, ..., then the same fold; one rounding to float at the end
__global__ void __launch_bounds__(256) graph_loss_finish_kernel(const float *__restrict__ partial, int nblocks, float scale,
                                                                float *__restrict__ loss)
{
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) s += (double)partial[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)((double)scale * ((red[0] + red[1]) + (red[2] + red[3])));
}

// ---- backward.  One lane per node: acc = 0; the own row in ascending k, acc += w * phi'(v[i] - v[target]); then the incoming
// edges in list order, acc -= w * phi'(v[source] - v[i]); grad = (g * scale) * acc.
// A node with more than GL_HUB incoming edges (a hub: everybody's nearest neighbour) would hold its whole wave up, so the wave
// sums its list together, hub after hub in ascending lane: lane l adds the list's entries l, l + 64, l + 128, ... in that order
// into p_l = 0 + ..., the 64 p_l are folded by xor butterfly (offsets 32, 16, .. 1; every lane ends with the same bits, addition
// being commutative), and the owner takes acc = acc - p.  Fixed by the list alone, so bit-reproducible like the serial path.
template <int KIND, bool HAS_W>
__device__ __forceinline__ float gl_incoming_term(int P, int K, uint32_t n, int e, float vi, const float *__restrict__ v,
                                                  const float *__restrict__ w, float delta)
{
    if ((uint32_t)e >= n) return 0.0f;   // (a list not made by r2_graph_transpose: nothing outside the inputs is read)
    float t = gl_dphi<KIND>(v[(uint32_t)e / (uint32_t)K], vi, delta);
    if (HAS_W) t = w[e] * t;
    return t;
}

template <int KIND, bool HAS_W>
__global__ void __launch_bounds__(GL_THREADS) graph_loss_bwd_kernel(int P, int K, uint32_t n, const float *__restrict__ v,
                                                                    const int *__restrict__ idx, const float *__restrict__ w,
                                                                    const int *__restrict__ in_offsets, const int *__restrict__ in_edges,
                                                                    float delta, float scale, const float *__restrict__ g,
                                                                    float *__restrict__ grad)
{
    const int i = blockIdx.x * GL_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = i < P;
    float acc = 0.0f, vi = 0.0f;
    bool any = false;
    int o0 = 0, o1 = 0;
    if (live) {
        vi = v[i];
        for (int k = 0; k < K; ++k) {
            const size_t e = (size_t)i * K + k;
            const int j = idx[e];
            if (j >= 0 && j < P) {
                float t = gl_dphi<KIND>(vi, v[j], delta);
                if (HAS_W) t = w[e] * t;
                acc += t;
                any = true;
            }
        }
        o0 = min(max(in_offsets[i], 0), (int)n);
        o1 = min(max(in_offsets[i + 1], o0), (int)n);
    }
    const bool hub = o1 - o0 > GL_HUB;
    if (!hub)
        for (int m = o0; m < o1; ++m) acc -= gl_incoming_term<KIND, HAS_W>(P, K, n, in_edges[m], vi, v, w, delta);
    unsigned long long hubs = __ballot(hub);
    while (hubs) {
        const int l = __ffsll((long long)hubs) - 1;
        hubs &= hubs - 1;
        const int h0 = __shfl(o0, l), h1 = __shfl(o1, l);
        const float hv = __shfl(vi, l);
        float p = 0.0f;
        for (int m = h0 + lane; m < h1; m += 64) p += gl_incoming_term<KIND, HAS_W>(P, K, n, in_edges[m], hv, v, w, delta);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) p += __shfl_xor(p, d);
        if (lane == l) acc = acc - p;
    }
    if (live) grad[i] = (any || o1 > o0) ? (g[0] * scale) * acc : 0.0f;   // a node without edges: exactly +0
}

inline size_t gl_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline bool gl_shape_ok(int P, int K) { return P >= 0 && K >= 1 && (size_t)P * (size_t)K <= 0x7fffffffu; }

template <int KIND, bool HAS_W>
void gl_launch_fwd(int nb, int P, int K, uint32_t n, const float *v, const int *idx, const float *w, float delta, float *partial,
                   hipStream_t s)
{
    graph_loss_fwd_kernel<KIND, HAS_W><<<dim3((unsigned)nb), dim3(GL_THREADS), 0, s>>>(P, K, n, v, idx, w, delta, partial);
}

template <int KIND, bool HAS_W>
void gl_launch_bwd(int P, int K, uint32_t n, const float *v, const int *idx, const float *w, const int *in_offsets,
                   const int *in_edges, float delta, float scale, const float *g, float *grad, hipStream_t s)
{
    graph_loss_bwd_kernel<KIND, HAS_W><<<dim3((unsigned)((P + GL_THREADS - 1) / GL_THREADS)), dim3(GL_THREADS), 0, s>>>(
        P, K, n, v, idx, w, in_offsets, in_edges, delta, scale, g, grad);
}

bool gl_kind_ok(const char *what, int kind, float delta)
{
    if (kind < R2_GRAPH_KIND_L1 || kind > R2_GRAPH_KIND_HUBER) {
        set_error("%s: kind %d is not 0 (l1), 1 (l2) or 2 (huber)", what, kind);
        return false;
    }
    if (kind == R2_GRAPH_KIND_HUBER && !(delta > 0.0f)) {
        set_error("%s: the Huber kind needs delta > 0, got %g", what, (double)delta);
        return false;
    }
    return true;
}

}  // namespace
}  // namespace r2

extern "C" size_t r2_graph_transpose_workspace_bytes(int P, int K)
{
    if (!r2::gl_shape_ok(P, K)) return 0;
    const size_t n = (size_t)P * (size_t)K;
    return 2 * r2::gl_align(n * sizeof(uint32_t)) + r2::gl_align(r2::sort_temp_bytes(n)) + 256;
}

extern "C" int r2_graph_transpose(int P, int K, const int *idx, int *in_offsets, int *in_edges, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    using namespace r2;
    if (!gl_shape_ok(P, K) || !in_offsets || (P > 0 && (!idx || !in_edges))) {
        set_error("r2_graph_transpose: invalid argument");
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)P * (size_t)K;
    const uint32_t *sorted_keys = nullptr;
    if (n > 0) {
        if (!workspace || workspace_bytes < r2_graph_transpose_workspace_bytes(P, K)) {
            set_error("r2_graph_transpose: the workspace must hold %zu bytes", r2_graph_transpose_workspace_bytes(P, K));
            return R2_ERR_INVALID;
        }
        char *ws = static_cast<char *>(workspace);
        uint32_t *keys = reinterpret_cast<uint32_t *>(ws);
        uint32_t *keys_out = reinterpret_cast<uint32_t *>(ws + gl_align(n * sizeof(uint32_t)));
        char *temp = ws + 2 * gl_align(n * sizeof(uint32_t));
        graph_keys_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(P, (uint32_t)n, idx, keys);
        // key bits: the values 0 .. P (P itself marks an invalid edge); the value of a pair is its input index = the edge id,
        // and the sort is stable, so equal targets keep ascending edge ids
        const int end_bit = 32 - __builtin_clz((unsigned)P);
        const int rc = sort_pairs_ex(temp, workspace_bytes - 2 * gl_align(n * sizeof(uint32_t)), keys, keys_out, nullptr,
                                     reinterpret_cast<uint32_t *>(in_edges), nullptr, nullptr, n, end_bit, false, nullptr, s);
        if (rc) return rc;
        sorted_keys = keys_out;
    }
    graph_offsets_kernel<<<dim3((unsigned)(P / 256 + 1)), dim3(256), 0, s>>>(P, (uint32_t)n, sorted_keys, in_offsets);
    R2_STAGE_CHECK(0, s, "graph transpose");
    return 0;
}

extern "C" size_t r2_graph_loss_scratch_floats(int P, int K)
{
    if (!r2::gl_shape_ok(P, K)) return 0;
    return std::max<size_t>(1, ((size_t)P * (size_t)K + r2::GL_BLOCK_EDGES - 1) / r2::GL_BLOCK_EDGES);
}

extern "C" int r2_graph_loss(int P, int K, const float *v, const int *idx, const float *w, int kind, float delta, float scale,
                             float *scratch, float *loss, void *stream)
{
    using namespace r2;
    if (!gl_shape_ok(P, K) || !scratch || !loss || (P > 0 && (!v || !idx))) {
        set_error("r2_graph_loss: invalid argument");
        return R2_ERR_INVALID;
    }
    if (!gl_kind_ok("r2_graph_loss", kind, delta)) return R2_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)((size_t)P * (size_t)K);
    const int nb = (int)((n + (uint32_t)GL_BLOCK_EDGES - 1) / (uint32_t)GL_BLOCK_EDGES);
    if (nb > 0) {
#define R2_GL_FWD(KIND)                                                                                              \
    (w ? gl_launch_fwd<KIND, true>(nb, P, K, n, v, idx, w, delta, scratch, s)                                        \
       : gl_launch_fwd<KIND, false>(nb, P, K, n, v, idx, w, delta, scratch, s))
        if (kind == R2_GRAPH_KIND_L1) R2_GL_FWD(R2_GRAPH_KIND_L1);
        else if (kind == R2_GRAPH_KIND_L2) R2_GL_FWD(R2_GRAPH_KIND_L2);
        else R2_GL_FWD(R2_GRAPH_KIND_HUBER);
#undef R2_GL_FWD
    }
    graph_loss_finish_kernel<<<dim3(1), dim3(256), 0, s>>>(scratch, nb, scale, loss);
    R2_STAGE_CHECK(0, s, "graph loss");
    return 0;
}

extern "C" int r2_graph_loss_backward(int P, int K, const float *v, const int *idx, const float *w, const int *in_offsets,
                                      const int *in_edges, int kind, float delta, float scale, const float *g, float *grad,
                                      void *stream)
{
    using namespace r2;
    if (!gl_shape_ok(P, K) || (P > 0 && (!v || !idx || !in_offsets || !in_edges || !g || !grad))) {
        set_error("r2_graph_loss_backward: invalid argument");
        return R2_ERR_INVALID;
    }
    if (!gl_kind_ok("r2_graph_loss_backward", kind, delta)) return R2_ERR_INVALID;
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)((size_t)P * (size_t)K);
#define R2_GL_BWD(KIND)                                                                                              \
    (w ? gl_launch_bwd<KIND, true>(P, K, n, v, idx, w, in_offsets, in_edges, delta, scale, g, grad, s)                \
       : gl_launch_bwd<KIND, false>(P, K, n, v, idx, w, in_offsets, in_edges, delta, scale, g, grad, s))
    if (kind == R2_GRAPH_KIND_L1) R2_GL_BWD(R2_GRAPH_KIND_L1);
    else if (kind == R2_GRAPH_KIND_L2) R2_GL_BWD(R2_GRAPH_KIND_L2);
    else R2_GL_BWD(R2_GRAPH_KIND_HUBER);
#undef R2_GL_BWD
    R2_STAGE_CHECK(0, s, "graph loss backward");
    return 0;
}
