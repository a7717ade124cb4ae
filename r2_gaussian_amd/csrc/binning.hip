// binning.hip -- prefix sum, tile-range detection and work-list construction shared by the rasterizer and the
// voxelizer.  Replaces cub::DeviceScan::InclusiveSum / identifyTileRanges of the reference
// (RAS/rasterizer_impl.cu:116-138,275,308-316); the sort lives in radix_sort.hip, the host runtime in host_runtime.hip.
#include "r2_common.hpp"

namespace r2 {

uint32_t higher_msb(uint32_t n)
{
    // smallest b with (n >> b) == 0, i.e. bit length of n (same value as the reference's
    // getHigherMsb binary search, RAS/rasterizer_impl.cu:35-50, for every n >= 1)
    uint32_t msb = 16, step = 16;
    while (step > 1) {
        step >>= 1;
        msb = (n >> msb) ? msb + step : msb - step;
    }
    if (n >> msb) msb++;
    return msb;
}

// ---- prefix sum (replaces cub::DeviceScan::InclusiveSum, RAS/rasterizer_impl.cu:275): two kernels, no
// inter-workgroup waiting.  K1: every workgroup reduces its 4096-element tile; K2: every workgroup adds up the
// partials of the tiles before it (<= a few hundred values) and scans its own tile.  `order` (optional) gathers the
// input: out[j] = sum_{i<=j} in[order[i]] -- the per-Gaussian tile counts visited in depth order.
constexpr int SC_THREADS = 1024;
constexpr int SC_IPT = 4;
constexpr int SC_TILE = SC_THREADS * SC_IPT;

__device__ __forceinline__ uint32_t block_reduce_1024(uint32_t v, uint32_t *sh /* [16] */)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < SC_THREADS / 64; ++w) t += sh[w];
    __syncthreads();
    return t;
}

__global__ void __launch_bounds__(SC_THREADS) scan_reduce_kernel(const uint32_t *__restrict__ in,
                                                                 const uint32_t *__restrict__ order, uint32_t n,
                                                                 uint32_t *__restrict__ partial)
{
    __shared__ uint32_t sh[SC_THREADS / 64];
    const uint32_t base = blockIdx.x * SC_TILE + threadIdx.x * SC_IPT;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < SC_IPT; ++i) {
        const uint32_t j = base + i;
        if (j < n) v += in[order ? order[j] : j];
    }
    const uint32_t t = block_reduce_1024(v, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ void __launch_bounds__(SC_THREADS) scan_apply_kernel(const uint32_t *__restrict__ in,
                                                                const uint32_t *__restrict__ order, uint32_t n,
                                                                const uint32_t *__restrict__ partial,
                                                                uint32_t *__restrict__ out, uint32_t *__restrict__ total_out)
{
    __shared__ uint32_t sh[SC_THREADS / 64];
    __shared__ uint32_t wsum[SC_THREADS / 64];
    uint32_t pre = 0;
    for (uint32_t g = threadIdx.x; g < blockIdx.x; g += SC_THREADS) pre += partial[g];
    const uint32_t tile_base = block_reduce_1024(pre, sh);
    const uint32_t base = blockIdx.x * SC_TILE + threadIdx.x * SC_IPT;
    uint32_t x[SC_IPT], sum = 0;
#pragma unroll
    for (int i = 0; i < SC_IPT; ++i) {
        const uint32_t j = base + i;
        x[i] = j < n ? in[order ? order[j] : j] : 0u;
        sum += x[i];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t run = tile_base + incl - sum;
    for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
    for (int i = 0; i < SC_IPT; ++i) {
        run += x[i];
        if (base + i < n) {
            out[base + i] = run;
            if (total_out && base + i == n - 1) *total_out = run;   // grand total, next to the other host-read words
        }
    }
}

size_t scan_temp_bytes(int P) { return sizeof(uint32_t) * ((size_t)(P + SC_TILE - 1) / SC_TILE + 32); }
size_t scan_gather_temp_bytes(int P) { return scan_temp_bytes(P); }

int inclusive_scan_gather_u32(void *temp, size_t temp_bytes, const uint32_t *in, const uint32_t *order, uint32_t *out,
                              int P, hipStream_t s, uint32_t *total_out)
{
    if (P <= 0) return 0;
    if (temp_bytes < scan_temp_bytes(P)) {
        set_error("inclusive_scan: temp storage too small");
        return R2_ERR_INVALID;
    }
    const uint32_t tiles = (uint32_t)((P + SC_TILE - 1) / SC_TILE);
    uint32_t *partial = reinterpret_cast<uint32_t *>(temp);
    scan_reduce_kernel<<<dim3(tiles), dim3(SC_THREADS), 0, s>>>(in, order, (uint32_t)P, partial);
    scan_apply_kernel<<<dim3(tiles), dim3(SC_THREADS), 0, s>>>(in, order, (uint32_t)P, partial, out, total_out);
    R2_HIP_TRY(hipGetLastError());
    return 0;
}

int inclusive_scan_u32(void *temp, size_t temp_bytes, const uint32_t *in, uint32_t *out, int P, hipStream_t s)
{
    return inclusive_scan_gather_u32(temp, temp_bytes, in, nullptr, out, P, s, nullptr);
}

// One thread per sorted instance; a tile boundary writes the end of the previous tile's range and the
// start of the next one.  ranges must be zeroed first (tiles with no instance keep (0,0)).
__global__ void __launch_bounds__(256) tile_ranges_kernel(const uint32_t *__restrict__ tiles,
                                                          const uint32_t *__restrict__ perm,
                                                          const uint32_t *__restrict__ vals_unsorted,
                                                          uint32_t *__restrict__ point_list, uint32_t L,
                                                          uint2 *__restrict__ ranges)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= L) return;
    if (point_list) point_list[idx] = vals_unsorted[perm[idx]];   // absent when the sort carried the ids itself
    const uint32_t cur = tiles[idx];
    if (idx == 0) ranges[cur].x = 0;
    else {
        const uint32_t prev = tiles[idx - 1];
        if (cur != prev) {
            ranges[prev].y = idx;
            ranges[cur].x = idx;
        }
    }
    if (idx == L - 1) ranges[cur].y = L;
}

int tile_ranges(const uint32_t *tiles_sorted, const uint32_t *perm, const uint32_t *vals_unsorted, uint32_t *point_list,
                size_t R, uint2 *ranges, size_t T, hipStream_t s, bool ranges_zeroed)
{
    if (!ranges_zeroed) R2_HIP_TRY(hipMemsetAsync(ranges, 0, T * sizeof(uint2), s));   // (else: an earlier kernel of the caller did it)
    if (R > 0)
        tile_ranges_kernel<<<dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s>>>(tiles_sorted, perm, vals_unsorted,
                                                                                  point_list, (uint32_t)R, ranges);
    return 0;
}

__global__ void __launch_bounds__(256) fill_tiles_kernel(const uint2 *__restrict__ ranges, uint32_t *__restrict__ tiles)
{
    const uint2 r = ranges[blockIdx.x];
    for (uint32_t k = r.x + threadIdx.x; k < r.y; k += 256) tiles[k] = blockIdx.x;
}
int fill_tiles_from_ranges(const uint2 *ranges, size_t T, uint32_t *tiles, hipStream_t s)
{
    if (T > 0) fill_tiles_kernel<<<dim3((unsigned)T), dim3(256), 0, s>>>(ranges, tiles);
    return 0;
}
// The tile lists are cut into work items of `chunk` instances for the render kernels (load balance).
// work list: tile t owns work items [chunk_base[t], chunk_base[t+1]).  One workgroup, T is small (<= 2^20).
__global__ void __launch_bounds__(1024) build_work_kernel(const uint2 *__restrict__ ranges, uint32_t T, uint32_t chunk,
                                                          uint32_t *__restrict__ chunk_base,
                                                          uint4 *__restrict__ work_tile, uint32_t min_len)
{
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < T; base += 1024) {
        const uint32_t t = base + tid;
        uint32_t n = 0;
        if (t < T) {
            const uint2 r = ranges[t];
            const uint32_t ch = work_tile_chunk(chunk, r.y - r.x);
            n = (r.y - r.x) < min_len ? 0u : (r.y - r.x + ch - 1) / ch;
        }
        // inclusive scan inside the wave, then across the 16 waves
        uint32_t incl = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t woff = 0;
        for (int w = 0; w < wave; ++w) woff += wsum[w];
        const uint32_t excl = carry + woff + incl - n;
        if (t < T) {
            chunk_base[t] = excl;
            const uint2 r = ranges[t];
            const uint32_t ch = work_tile_chunk(chunk, r.y - r.x);
            for (uint32_t j = 0; j < n; ++j)   // work descriptor: {tile, first instance, one past the last, items of the tile}
                work_tile[excl + j] = make_uint4(t, r.x + j * ch, min(r.y, r.x + (j + 1) * ch), n);
        }
        __syncthreads();
        if (tid == 1023) carry = excl + n;
        __syncthreads();
    }
    if (tid == 0) chunk_base[T] = carry;
}

// (Measured and left out, round 4: ONE workgroup for 32768 tiles as well, every thread owning 32 consecutive tiles, two passes over
// the L2-resident ranges with eight loads in flight -- one launch instead of four, but 45 us slower: 43 k stores through one CU.)
// many tiles (256^3 volume: 32768): the same in TWO launches -- a scan whose two kernels compute the per-tile work item counts from
// the ranges themselves, and whose second one writes bases and work items on the way (count + scan-reduce, scan-apply + fill)
__device__ __forceinline__ uint32_t work_items_of(const uint2 r, uint32_t chunk, uint32_t min_len)
{
    const uint32_t len = r.y - r.x, ch = work_tile_chunk(chunk, len);
    return len < min_len ? 0u : (len + ch - 1) / ch;
}
__global__ void __launch_bounds__(SC_THREADS) work_reduce_kernel(const uint2 *__restrict__ ranges, uint32_t T, uint32_t chunk,
                                                                 uint32_t min_len, uint32_t *__restrict__ partial)
{
    __shared__ uint32_t sh[SC_THREADS / 64];
    const uint32_t base = blockIdx.x * SC_TILE + threadIdx.x * SC_IPT;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < SC_IPT; ++i)
        if (base + i < T) v += work_items_of(ranges[base + i], chunk, min_len);
    const uint32_t t = block_reduce_1024(v, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}
__global__ void __launch_bounds__(SC_THREADS) work_apply_fill_kernel(const uint2 *__restrict__ ranges, uint32_t T, uint32_t chunk,
                                                                     uint32_t min_len, const uint32_t *__restrict__ partial,
                                                                     uint32_t *__restrict__ chunk_base, uint4 *__restrict__ work_tile)
{
    __shared__ uint32_t sh[SC_THREADS / 64];
    __shared__ uint32_t wsum[SC_THREADS / 64];
    uint32_t pre = 0;
    for (uint32_t g = threadIdx.x; g < blockIdx.x; g += SC_THREADS) pre += partial[g];
    const uint32_t tile_base = block_reduce_1024(pre, sh);
    const uint32_t base = blockIdx.x * SC_TILE + threadIdx.x * SC_IPT;
    uint2 r[SC_IPT];
    uint32_t x[SC_IPT], sum = 0;
#pragma unroll
    for (int i = 0; i < SC_IPT; ++i) {
        r[i] = base + i < T ? ranges[base + i] : make_uint2(0u, 0u);
        x[i] = base + i < T ? work_items_of(r[i], chunk, min_len) : 0u;
        sum += x[i];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t run = tile_base + incl - sum;
    for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
    for (int i = 0; i < SC_IPT; ++i) {
        const uint32_t t = base + i;
        if (t < T) {
            chunk_base[t] = run;
            const uint32_t ch = work_tile_chunk(chunk, r[i].y - r[i].x);
            for (uint32_t j = 0; j < x[i]; ++j)   // work descriptor: {tile, first instance, one past the last, items of the tile}
                work_tile[run + j] = make_uint4(t, r[i].x + j * ch, min(r[i].y, r[i].x + (j + 1) * ch), x[i]);
            run += x[i];
            if (t == T - 1) chunk_base[T] = run;
        }
    }
}

// the second half of the two-launch construction alone, for a caller whose own kernels have left the per-block work item counts
// (partial[b] = work items of tiles [b * build_work_block_tiles(), ...)) -- voxel_sticks.hip: its sort kernel knows every tile's length
uint32_t build_work_block_tiles() { return (uint32_t)SC_TILE; }
void launch_build_work_from_partials(const uint2 *ranges, uint32_t T, uint32_t chunk, uint32_t *chunk_base, uint4 *work_tile,
                                     const uint32_t *partial, hipStream_t s, uint32_t min_len)
{
    const uint32_t tiles = (T + SC_TILE - 1) / SC_TILE;
    work_apply_fill_kernel<<<dim3(tiles), dim3(SC_THREADS), 0, s>>>(ranges, T, chunk, min_len, partial, chunk_base, work_tile);
}

size_t build_work_temp_bytes(size_t T) { return T > 4096 ? sizeof(uint32_t) * ((T + SC_TILE - 1) / SC_TILE) + 256 : 0; }

void launch_build_work(const uint2 *ranges, uint32_t T, uint32_t chunk, uint32_t *chunk_base, uint4 *work_tile,
                       void *temp, hipStream_t s, uint32_t min_len)
{
    if (T <= 4096 || temp == nullptr) {
        build_work_kernel<<<dim3(1), dim3(1024), 0, s>>>(ranges, T, chunk, chunk_base, work_tile, min_len);
        return;
    }
    uint32_t *partial = reinterpret_cast<uint32_t *>(temp);   // one word per block of SC_TILE tiles
    const uint32_t tiles = (T + SC_TILE - 1) / SC_TILE;
    work_reduce_kernel<<<dim3(tiles), dim3(SC_THREADS), 0, s>>>(ranges, T, chunk, min_len, partial);
    work_apply_fill_kernel<<<dim3(tiles), dim3(SC_THREADS), 0, s>>>(ranges, T, chunk, min_len, partial, chunk_base, work_tile);
}

// Single-pass tile sort: the sort's digit totals are the per-tile instance counts, so the tile ranges
// (identifyTileRanges, RAS/rasterizer_impl.cu:116-138) are their exclusive scan -- computed here together with the
// forward work list, by one workgroup (T <= 4096).
__global__ void __launch_bounds__(1024) ranges_and_work_kernel(const uint32_t *__restrict__ counts, WorkListOut wo)
{
    ranges_and_work_block<1024>(counts, wo);
}

void launch_ranges_and_work(const uint32_t *tile_counts, uint32_t T, uint32_t chunk, uint2 *ranges, uint32_t *chunk_base,
                            uint4 *work_tile, hipStream_t s, uint32_t min_len)
{
    ranges_and_work_kernel<<<dim3(1), dim3(1024), 0, s>>>(tile_counts, WorkListOut{ranges, chunk_base, work_tile, T, chunk, nullptr, min_len});
}

}  // namespace r2
