// gaussian_skeleton.hpp -- the kernel skeletons of the exact operators on the Gaussian cloud, written once, on top of
// gaussian_rays.hpp.  Every property those operators advertise -- a pair is differentiated exactly when the forward summed
// it, a thread adds its pairs in ascending index, the same bits come out on every call -- lives in the five pieces below;
// the kernels hand them small callables (lambdas) for the lines in which they differ.
//
//   the loaded Gaussian   Cloud / CloudOut, Gauss, load_gauss, store_gauss: the only reads and writes of the parameter arrays;
//   the gather round      gather_rounds: P Gaussians NT at a time, hit test, in-order compaction into an LDS batch, every
//                         active thread walks the batch (the pixel-tile kernels through pixel_tile and tile_rounds);
//   the list round        TileLists, list_rounds: the same batch and the same walk, fed from a tile's list of a projection
//                         plan instead of the cloud (tile_rounds on TileLists): one staging per list entry, no test;
//   the tile prologue     PixelTile, pixel_tile: the tile's bounds, the thread's pixel and its ray, the view's constants;
//   the Gaussian wave     gauss_wave: one wave per Gaussian, eleven sums per lane, one butterfly, one store; with rect_walk
//                         (the pixels of the Gaussian's rectangle) or hit_block_walk (the blocks whose box meets its sphere).
//
// The host part at the end holds the argument checks the entry points share.
#pragma once
#include "gaussian_rays.hpp"

namespace r2 {

constexpr int NPAR = 11;   // parameters of a Gaussian: mean (3), density, scales (3), quaternion (4), in gauss_pair_grad's order

// The cloud as the kernels take it, by value: P Gaussians, their four parameter arrays and the scale modifier.
struct Cloud {
    int P;
    const float *means, *density, *scales;
    float mod;
    const float *rotations;
    bool missing() const { return P > 0 && (!means || !density || !scales || !rotations); }   // host: an array is absent
};

// One array of NPAR numbers per Gaussian, split as the parameters are: gradients, Fisher rows (written) or variances (read).
struct CloudOut {
    float *means, *density, *scales, *rotations;
    bool missing(int P) const { return P > 0 && (!means || !density || !scales || !rotations); }
};

// One Gaussian's parameters as they lie in memory: the unmodified scales, the quaternion as given.
struct Gauss {
    float mx, my, mz, rho;
    float s[3];
    float4 q;
};

__device__ __forceinline__ Gauss load_gauss(const Cloud &c, int i)
{
    Gauss g;
    g.mx = c.means[3 * i]; g.my = c.means[3 * i + 1]; g.mz = c.means[3 * i + 2];
    g.rho = c.density[i];
    g.s[0] = c.scales[3 * i]; g.s[1] = c.scales[3 * i + 1]; g.s[2] = c.scales[3 * i + 2];
    g.q = make_float4(c.rotations[4 * i], c.rotations[4 * i + 1], c.rotations[4 * i + 2], c.rotations[4 * i + 3]);
    return g;
}

__device__ __forceinline__ void store_gauss(const CloudOut &d, int i, const float *acc)
{
    float *m = d.means + 3 * i, *s = d.scales + 3 * i, *q = d.rotations + 4 * i;
    m[0] = acc[0]; m[1] = acc[1]; m[2] = acc[2];
    d.density[i] = acc[3];
    s[0] = acc[4]; s[1] = acc[5]; s[2] = acc[6];
    q[0] = acc[7]; q[1] = acc[8]; q[2] = acc[9]; q[3] = acc[10];
}

__device__ __forceinline__ float gauss_radius(const Gauss &a, float mod)
{
    return gauss_radius(a.mx, a.my, a.mz, a.rho, a.s[0], a.s[1], a.s[2], mod, a.q);
}

__device__ __forceinline__ GaussRec gauss_rec(const Gauss &a, float mod)
{
    return gauss_rec(a.mx, a.my, a.mz, a.rho, a.s[0], a.s[1], a.s[2], mod, a.q);
}

// The in-order gather round.  The NT threads of the workgroup walk the cloud NT Gaussians at a time: thread i loads Gaussian
// base + i, and hit(a, radius) decides whether the workgroup needs it (radius >= 0 is tested here); the hits are compacted
// IN ORDER (wave ballots + the wave counts) into the LDS batch st through stage(st[slot], a, radius, i), and every thread
// with `active` set then calls consume(st[j]) for the batch in order: it sees the Gaussians it needs in ascending index.
// `active` is a value and never an early return: every thread of the workgroup reaches both barriers of every round.
template <int NT, typename Rec, typename Hit, typename Stage, typename Consume>
__device__ __forceinline__ void gather_rounds(const Cloud &cl, Rec *st, bool active, Hit hit_test, Stage stage, Consume consume)
{
    __shared__ int wcount[NT / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    for (int base = 0; base < cl.P; base += NT) {
        const int i = base + tid;
        bool hit = false;
        Gauss a = {};
        float radius = 0.f;
        if (i < cl.P) {
            a = load_gauss(cl, i);
            radius = gauss_radius(a, cl.mod);
            hit = radius >= 0.0f && hit_test(a, radius);
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) wcount[wave] = __popcll(mask);
        __syncthreads();
        int slot = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < NT / WAVE; ++w) {
            if (w < wave) slot += wcount[w];
            total += wcount[w];
        }
        if (hit) stage(st[slot], a, radius, i);
        __syncthreads();
        if (active)
            for (int j = 0; j < total; ++j) consume(st[j]);
        __syncthreads();   // the batch and the wave counts are rewritten by the next round
    }
}

// What a thread of a 16 x 16 pixel tile knows before the rounds: the tile (blockIdx.x, blockIdx.y) of view blockIdx.z, cut to
// the detector, its own pixel, whether that lies on the detector, the view's twelve numbers and the pixel's ray.
struct PixelTile {
    int view, tc0, tr0, tc1, tr1, c, r;
    bool inside;
    const float *R;
    Ray y;
    float len;
};

// All threads of the workgroup call it: thread 0 writes the view's constants to vg (LDS), and a barrier follows.
__device__ __forceinline__ PixelTile pixel_tile(const float *__restrict__ rays, int cone, int H, int W, ViewGeom &vg)
{
    PixelTile t;
    const int tid = threadIdx.x;
    t.view = blockIdx.z;
    t.tc0 = blockIdx.x * TILE2D; t.tr0 = blockIdx.y * TILE2D;
    t.tc1 = min(t.tc0 + TILE2D, W) - 1; t.tr1 = min(t.tr0 + TILE2D, H) - 1;
    t.c = t.tc0 + (tid & (TILE2D - 1)); t.r = t.tr0 + tid / TILE2D;
    t.inside = t.c < W && t.r < H;
    t.R = rays + 12 * t.view;
    if (tid == 0) vg = view_geom(t.R, cone);
    __syncthreads();
    t.y = pixel_ray(t.R, cone, t.r, t.c);
    t.len = ray_length(t.y);
    return t;
}

// What the projector's forward and its ray backward stage of a Gaussian whose rectangle meets the tile.
struct Staged {
    GaussRec g;
    PixRect q;
};

// The gather round of the pixel-tile kernels: a Gaussian is a hit when its detector rectangle (gauss_rect) meets the tile;
// stage(st[slot], a, i) fills the record, whose member q receives the rectangle here, and a pixel on the detector calls
// pair(st[j]) for the batch's Gaussians whose rectangle holds it.
template <typename Rec, typename Stage, typename Pair>
__device__ __forceinline__ void tile_rounds(const Cloud &cl, const PixelTile &t, const ViewGeom &vg, int cone, int H, int W, Rec *st,
                                            Stage stage, Pair pair)
{
    PixRect rc;
    gather_rounds<TILE2D * TILE2D>(
        cl, st, t.inside,
        [&](const Gauss &a, float radius) {
            return gauss_rect(vg, cone, a.mx, a.my, a.mz, radius, H, W, rc) && rc.c0 <= t.tc1 && rc.c1 >= t.tc0 && rc.r0 <= t.tr1 &&
                   rc.r1 >= t.tr0;
        },
        [&](Rec &d, const Gauss &a, float, int i) {
            stage(d, a, i);
            d.q = rc;
        },
        [&](const Rec &s) {
            if (t.c < s.q.c0 || t.c > s.q.c1 || t.r < s.q.r0 || t.r > s.q.r1) return;
            pair(s);
        });
}

// The per-tile lists of a projection plan (gaussian_plan.hip builds them; include/r2hip.h has the layout): list k = (view T +
// ty Tx + tx) is ids[offsets[k] .. offsets[k + 1]), ascending Gaussian indices, and `capacity` is the number of ints `ids`
// holds.  THE LISTS DRIVE THE KERNEL: a Gaussian that is not in a tile's list contributes nothing to that tile, whatever its
// rectangle, so a caller may hand in lists of their own.
struct TileLists {
    const long long *offsets;
    const int *ids;
    long long capacity;
};

// Where the pixel-tile kernels take their Gaussians from: the whole cloud (gather_rounds) or the tile's list (list_rounds).
struct WholeCloud {};

// The list-driven round: entries [beg, end) of ids, NT at a time.  Thread i stages entry base + i into st[i] through
// stage(st[i], id) -- no ballot and no compaction, every entry is a hit and the list's order is the batch's -- and every
// thread with `active` set then calls consume(st[j]) for the batch in order.  Two barriers per round, which every thread of
// the workgroup reaches.
template <int NT, typename Rec, typename Stage, typename Consume>
__device__ __forceinline__ void list_rounds(const int *__restrict__ ids, long long beg, long long end, Rec *st, bool active,
                                            Stage stage, Consume consume)
{
    const int tid = threadIdx.x;
    for (long long base = beg; base < end; base += NT) {
        const int total = end - base < NT ? (int)(end - base) : NT;
        if (tid < total) stage(st[tid], ids[base + tid]);
        __syncthreads();
        if (active)
            for (int j = 0; j < total; ++j) consume(st[j]);
        __syncthreads();   // the batch is rewritten by the next round
    }
}

// tile_rounds on the whole cloud, and on the tile's list: an entry is staged as the gather round stages a hit -- its radius
// and rectangle are computed again, by the same functions, and stage(st[i], a, id) fills the same record -- so a pixel adds
// the pairs it adds without a plan, in the same order, and the same bits come out.  A list's ends are clamped to the
// buffer's capacity; an entry that is no index of the cloud, or a Gaussian without radius or rectangle, is staged with an
// empty rectangle that holds no pixel.
template <typename Rec, typename Stage, typename Pair>
__device__ __forceinline__ void tile_rounds(const WholeCloud &, const Cloud &cl, const PixelTile &t, const ViewGeom &vg, int cone,
                                            int H, int W, Rec *st, Stage stage, Pair pair)
{
    tile_rounds(cl, t, vg, cone, H, W, st, stage, pair);
}

template <typename Rec, typename Stage, typename Pair>
__device__ __forceinline__ void tile_rounds(const TileLists &tl, const Cloud &cl, const PixelTile &t, const ViewGeom &vg, int cone,
                                            int H, int W, Rec *st, Stage stage, Pair pair)
{
    const size_t k = ((size_t)t.view * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const long long beg = min(max(tl.offsets[k], 0ll), tl.capacity), end = min(max(tl.offsets[k + 1], beg), tl.capacity);
    list_rounds<TILE2D * TILE2D>(
        tl.ids, beg, end, st, t.inside,
        [&](Rec &d, int i) {
            d.q = PixRect{ 1, 0, 1, 0 };
            if (i < 0 || i >= cl.P) return;
            const Gauss a = load_gauss(cl, i);
            const float radius = gauss_radius(a, cl.mod);
            PixRect rc;
            if (!(radius >= 0.0f) || !gauss_rect(vg, cone, a.mx, a.my, a.mz, radius, H, W, rc)) return;
            stage(d, a, i);
            d.q = rc;
        },
        [&](const Rec &s) {
            if (t.c < s.q.c0 || t.c > s.q.c1 || t.r < s.q.r0 || t.r > s.q.r1) return;
            pair(s);
        });
}

// The Gaussian-major wave: wave w of workgroup b owns Gaussian i = b NT / 64 + w.  It loads the Gaussian, and when the Gaussian
// has a radius, walk(a, g, radius, lane, acc) adds the lane's pairs to its NPAR sums; one xor butterfly then adds the 64
// partial sums in a fixed order and lane 0 writes row i of out.  A Gaussian without a radius, or one that the walk finds
// nothing for, gets exact zeros.  No barrier: the waves of a workgroup do not meet.
template <int NT, typename Walk>
__device__ __forceinline__ void gauss_wave(const Cloud &cl, const CloudOut &out, Walk walk)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int i = blockIdx.x * (NT / WAVE) + threadIdx.x / WAVE;   // wave-uniform
    if (i >= cl.P) return;
    const Gauss a = load_gauss(cl, i);
    float acc[NPAR];
#pragma unroll
    for (int k = 0; k < NPAR; ++k) acc[k] = 0.0f;
    const float radius = gauss_radius(a, cl.mod);
    if (radius >= 0.0f) walk(a, gauss_rec(a, cl.mod), radius, lane, acc);
#pragma unroll
    for (int t = 0; t < NPAR; ++t)
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) acc[t] += __shfl_xor(acc[t], d);
    if (lane == 0) store_gauss(out, i, acc);
}

// The walk over the detector: for each view in order the Gaussian's rectangle -- the one the forward took -- row-major, lane l
// taking pixels l, l + 64, ...; pair(y, p, pix) is called for every pair gauss_pair accepts, pix = (view H + r) W + c.
template <typename Pair>
__device__ __forceinline__ void rect_walk(int V, int H, int W, const float *__restrict__ rays, int cone, const Gauss &a,
                                          const GaussRec &g, float radius, int lane, Pair pair)
{
    for (int view = 0; view < V; ++view) {
        const float *R = rays + 12 * view;
        const ViewGeom vg = view_geom(R, cone);
        PixRect rc;
        if (!gauss_rect(vg, cone, a.mx, a.my, a.mz, radius, H, W, rc)) continue;
        const int nw = rc.c1 - rc.c0 + 1, n = nw * (rc.r1 - rc.r0 + 1);   // <= H W < 2^30 (checked by the host)
        const size_t first = (size_t)view * H * W;
        for (int k = lane; k < n; k += WAVE) {
            const int rr = k / nw, r = rc.r0 + rr, c = rc.c0 + (k - rr * nw);
            const Ray y = pixel_ray(R, cone, r, c);
            GaussPair p;
            if (gauss_pair(g, y, cone, p)) pair(y, p, first + (size_t)r * W + c);
        }
    }
}

// The walk over N items (points, rays) that come in NB blocks of BLK consecutive ones, each block with a box: the wave tests
// the blocks 64 at a time, meets(b) saying whether block b's box meets the Gaussian's sphere, and walks the blocks that do in
// ascending order, lane l calling item(n) for items l, l + 64, ... of the block.
template <int BLK, typename Meets, typename Item>
__device__ __forceinline__ void hit_block_walk(int N, int NB, int lane, Meets meets, Item item)
{
    for (int base = 0; base < NB; base += WAVE) {
        const int b = base + lane;
        unsigned long long mask = __ballot(b < NB && meets(b < NB ? b : 0));
        while (mask) {   // wave-uniform: the blocks that meet the sphere, ascending
            const int hit = base + __ffsll((long long)mask) - 1;
            mask &= mask - 1ull;
#pragma unroll 1
            for (int k = 0; k < BLK / WAVE; ++k) {
                const long long n = (long long)hit * BLK + k * WAVE + lane;
                if (n < N) item(n);
            }
        }
    }
}

// ---- host: the argument checks the entry points share.  Each sets the error text, which names the entry point; the bool
// ones return true when the call is to be refused with R2_ERR_INVALID.
inline int invalid_argument(const char *entry)
{
    set_error("%s: invalid argument", entry);
    return R2_ERR_INVALID;
}

// The lists of a planned entry point: P = 0 needs none; a capacity of 0 needs no ids (every list is then empty).
inline bool lists_missing(int P, const TileLists &tl)
{
    return tl.capacity < 0 || (P > 0 && (!tl.offsets || (tl.capacity > 0 && !tl.ids)));
}

constexpr int CLOUD_MAX_P = 1 << 29;

inline bool cloud_too_large(const char *entry, int P)
{
    if (P <= CLOUD_MAX_P) return false;
    set_error("%s: shape out of range (P %d)", entry, P);
    return true;
}

// sizer: the name of the function that tells the caller how many bytes are needed.
inline bool workspace_too_small(const char *entry, const char *sizer, const void *workspace, size_t workspace_bytes, size_t need)
{
    if (need == 0 || (workspace && workspace_bytes >= need)) return false;
    set_error("%s: workspace of %zu bytes, %zu needed (%s)", entry, workspace ? workspace_bytes : (size_t)0, need, sizer);
    return true;
}

}  // namespace r2
