// isosurface.hip -- the level set {vol = level} of a volume [nx][ny][nz] as an indexed triangle mesh, by marching tetrahedra on
// the Kuhn (Freudenthal) subdivision of the voxel lattice (mesh.py: isosurface, model_isosurface).  include/r2hip.h states the
// contract (r2_isosurface_count); tests/isosurface_ref.py restates it in float32 operation for operation, which is why this
// file is compiled without FMA contraction.
//
// A cell is cut into the six tetrahedra 000 -> +e_a -> +e_a+e_b -> 111, one per permutation (a, b, c) of the axes.  Every edge
// of every tetrahedron runs from a lattice point p to p + d, d in {0,1}^3 \ {0}; p owns it, and its direction code is
// c = dx + 2 dy + 4 dz.  The only table is the 16 sign cases of one tetrahedron (tet_case below).
//
// Points are dealt in their linear order (z fastest): a workgroup of TB threads takes PPB consecutive points, each of its
// waves a run of PPW = ITER * 64 of them, 64 consecutive points per load.  All prefix sums are: the wave's ITER values,
// one exchange of the wave totals through LDS, a shuffle scan per 64 points -- no atomics, so two calls give the
// same bytes.
//   count:  iso_count_kernel   one read of the volume: per point the 7-bit mask of its crossed owned edges and its cell's
//                              triangle count (a byte each, into the workspace); per workgroup the sums of both and the
//                              number of invalid values
//           iso_scan_kernel    one workgroup: the exclusive prefix of the workgroup sums, and the three totals
//           iso_base_kernel    mask -> the int32 id of every owner's first vertex (written where the mask is not empty)
//   fill:   iso_vertex_kernel  mask, base -> vertices and normals (four points per thread; the volume is read at the
//                              crossed edges only)
//           iso_face_kernel    triangle counts -> every cell's offset; a wave lists its cells with triangles in LDS and
//                              deals them over its lanes; such a cell reads its 8 corners and the mask and base of its
//                              7 owners, and emits
#include "r2_common.hpp"
#include <math.h>

namespace r2 {

namespace {

constexpr int TB = 256;                   // threads per workgroup
constexpr int ITER = 16;                  // points per thread
constexpr int PPW = ITER * WAVE;          // points per wave: consecutive
constexpr int PPB = PPW * (TB / WAVE);    // points per workgroup
constexpr int SCAN = 256;                 // threads of the one workgroup that scans the workgroup sums
constexpr float INVALID_ABOVE = 1e38f;

struct Lattice {
    int nx, ny, nz;
    unsigned sx, sy;   // strides of x and y in points (z is contiguous)
    unsigned N;        // points (< 2^31)
    int cells;         // every dimension >= 2
};

struct Work {   // the workspace, as r2_isosurface_count leaves it
    int *cnt_v, *cnt_t, *cnt_i;       // [nb] per workgroup: vertices, triangles, invalid values
    long long *off_v, *off_t;         // [nb] their exclusive prefixes
    unsigned char *mask, *tcnt;       // [N]
    int *base;                        // [N], defined where mask != 0
    size_t bytes;
};

unsigned blocks_of(unsigned N) { return (N + PPB - 1) / PPB; }

Work carve(void *ws, unsigned N)
{
    Bump b((char *)ws);
    const unsigned nb = blocks_of(N);
    Work w;
    w.cnt_v = b.take<int>(nb);
    w.cnt_t = b.take<int>(nb);
    w.cnt_i = b.take<int>(nb);
    w.off_v = b.take<long long>(nb);
    w.off_t = b.take<long long>(nb);
    w.mask = b.take<unsigned char>(N);
    w.tcnt = b.take<unsigned char>(N);
    w.base = b.take<int>(N);
    w.bytes = b.total();
    return w;
}

__device__ __forceinline__ void unflatten(const Lattice &g, unsigned L, int &i, int &j, int &k)
{
    k = (int)(L % (unsigned)g.nz);
    j = (int)((L / (unsigned)g.nz) % (unsigned)g.ny);
    i = (int)(L / g.sx);
}

// the first point of this wave's run, and the point of (iteration q, this lane)
__device__ __forceinline__ unsigned wave_first() { return blockIdx.x * (unsigned)PPB + (threadIdx.x / WAVE) * (unsigned)PPW; }

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ int wave_inclusive(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// The sum of the waves before this one in the workgroup; total: this wave's sum (wave-uniform).  Every thread calls it.
__device__ __forceinline__ int waves_before(int total)
{
    __shared__ int wsum[TB / WAVE];
    const int wave = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) wsum[wave] = total;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int w = 0; w < TB / WAVE; ++w)
        if (w < wave) before += wsum[w];
    return before;
}

// corners of the six tetrahedra (corner id = dx + 2 dy + 4 dz); odd permutations are mirrored
__device__ __forceinline__ constexpr int tet_corner(int t, int v)
{
    constexpr int PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    return v == 0 ? 0 : v == 1 ? (1 << PERM[t][0]) : v == 2 ? ((1 << PERM[t][0]) | (1 << PERM[t][1])) : 7;
}
__device__ __forceinline__ constexpr bool tet_mirrored(int t) { return t == 1 || t == 2 || t == 5; }

// ---- count -------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(TB) iso_count_kernel(Lattice g, const float *__restrict__ vol, float level, Work w)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned first = wave_first();
    int nv = 0, nt = 0, ni = 0;
#pragma unroll 4
    for (int q = 0; q < ITER; ++q) {
        const unsigned L = first + (unsigned)q * WAVE + lane;
        if (L >= g.N) break;
        int i, j, k;
        unflatten(g, L, i, j, k);
        const bool ex = g.cells && i + 1 < g.nx, ey = g.cells && j + 1 < g.ny, ez = g.cells && k + 1 < g.nz;
        const size_t o = L;
        const size_t dx = ex ? g.sx : 0, dy = ey ? g.sy : 0, dz = ez ? 1 : 0;
        // an end that does not exist is read at a point whose edge to it is not crossed
        const float f0 = vol[o];
        const float f1 = vol[o + dx], f2 = vol[o + dy], f3 = vol[o + dx + dy];
        const float f4 = vol[o + dz], f5 = vol[o + dx + dz], f6 = vol[o + dy + dz], f7 = vol[o + dx + dy + dz];
        ni += !(fabsf(f0) <= INVALID_ABOVE);
        const unsigned in0 = f0 >= level;
        const unsigned in = in0 | (unsigned)(f1 >= level) << 1 | (unsigned)(f2 >= level) << 2 | (unsigned)(f3 >= level) << 3 |
                            (unsigned)(f4 >= level) << 4 | (unsigned)(f5 >= level) << 5 | (unsigned)(f6 >= level) << 6 |
                            (unsigned)(f7 >= level) << 7;
        // bit c - 1: the edge of direction code c is crossed ...
        unsigned m = ((in0 ? ~in : in) >> 1) & 0x7fu;
        // ... and exists: every axis of its direction does
        const unsigned okx = ex ? 0x7fu : 0x2au;   // codes 2, 4, 6 have dx = 0
        const unsigned oky = ey ? 0x7fu : 0x19u;   // codes 1, 4, 5 have dy = 0
        const unsigned okz = ez ? 0x7fu : 0x07u;   // codes 1, 2, 3 have dz = 0
        m &= okx & oky & okz;
        int t = 0;
        if (ex && ey && ez && in != 0u && in != 0xffu) {
#pragma unroll
            for (int tet = 0; tet < 6; ++tet) {
                const int n = (int)((in >> tet_corner(tet, 0)) & 1u) + (int)((in >> tet_corner(tet, 1)) & 1u) +
                              (int)((in >> tet_corner(tet, 2)) & 1u) + (int)((in >> tet_corner(tet, 3)) & 1u);
                t += (n == 0 || n == 4) ? 0 : (n == 2 ? 2 : 1);
            }
        }
        w.mask[L] = (unsigned char)m;
        w.tcnt[L] = (unsigned char)t;
        nv += __popc(m);
        nt += t;
    }
    nv = wave_sum(nv);
    nt = wave_sum(nt);
    ni = wave_sum(ni);
    __shared__ int sums[3][TB / WAVE];
    if (lane == 0) {
        sums[0][threadIdx.x / WAVE] = nv;
        sums[1][threadIdx.x / WAVE] = nt;
        sums[2][threadIdx.x / WAVE] = ni;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < TB / WAVE; ++k) s += sums[threadIdx.x][k];
        (threadIdx.x == 0 ? w.cnt_v : threadIdx.x == 1 ? w.cnt_t : w.cnt_i)[blockIdx.x] = s;
    }
}

// One workgroup: thread t owns the chunk [t c, (t + 1) c) of the workgroup sums, adds it, the workgroup scans the SCAN chunk
// sums, and the thread writes its chunk's exclusive prefixes (csrc/gaussian_plan.hip: gaussian_plan_scan_kernel).
__global__ void __launch_bounds__(SCAN) iso_scan_kernel(unsigned nb, Work w, long long *__restrict__ counts)
{
    __shared__ long long sums[3][SCAN];
    const int tid = threadIdx.x;
    const unsigned c = (nb + SCAN - 1) / SCAN, lo = min((unsigned)tid * c, nb), hi = min(lo + c, nb);
    long long sv = 0, st = 0, si = 0;
#pragma unroll 8
    for (unsigned k = lo; k < hi; ++k) {
        sv += w.cnt_v[k];
        st += w.cnt_t[k];
        si += w.cnt_i[k];
    }
    sums[0][tid] = sv;
    sums[1][tid] = st;
    sums[2][tid] = si;
    __syncthreads();
    for (int d = 1; d < SCAN; d <<= 1) {   // inclusive scan of the chunk sums
        const long long a = tid >= d ? sums[0][tid - d] : 0, b = tid >= d ? sums[1][tid - d] : 0,
                        e = tid >= d ? sums[2][tid - d] : 0;
        __syncthreads();
        sums[0][tid] += a;
        sums[1][tid] += b;
        sums[2][tid] += e;
        __syncthreads();
    }
    long long rv = sums[0][tid] - sv, rt = sums[1][tid] - st;
#pragma unroll 8
    for (unsigned k = lo; k < hi; ++k) {
        w.off_v[k] = rv;
        w.off_t[k] = rt;
        rv += w.cnt_v[k];
        rt += w.cnt_t[k];
    }
    if (tid == SCAN - 1) {
        counts[0] = sums[0][tid];
        counts[1] = sums[1][tid];
        counts[2] = sums[2][tid];
    }
}

// The exclusive prefix, in point order, of a byte per point (LOAD(L); 0 beyond the lattice) on top of off[workgroup]:
// vals[q] and pre[q] for the point of (iteration q, this lane).  Every thread of the workgroup calls it.
template <typename Map>
__device__ __forceinline__ void point_prefix(const Lattice &g, const unsigned char *__restrict__ bytes, Map map,
                                             const long long *__restrict__ off, int (&vals)[ITER], long long (&pre)[ITER])
{
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned first = wave_first();
    int mine = 0;
#pragma unroll
    for (int q = 0; q < ITER; ++q) {
        const unsigned L = first + (unsigned)q * WAVE + lane;
        vals[q] = L < g.N ? (int)bytes[L] : 0;
        mine += map(vals[q]);
    }
    const int before = waves_before(wave_sum(mine));
    long long run = off[blockIdx.x] + before;
#pragma unroll
    for (int q = 0; q < ITER; ++q) {
        const int v = map(vals[q]), incl = wave_inclusive(v, lane);
        pre[q] = run + (incl - v);
        run += __shfl(incl, WAVE - 1);
    }
}

__global__ void __launch_bounds__(TB) iso_base_kernel(Lattice g, Work w)
{
    int m[ITER];
    long long pre[ITER];
    point_prefix(g, w.mask, [](int v) { return __popc((unsigned)v); }, w.off_v, m, pre);
    const unsigned first = wave_first() + (threadIdx.x & (WAVE - 1));
#pragma unroll
    for (int q = 0; q < ITER; ++q)
        if (m[q] != 0) w.base[first + (unsigned)q * WAVE] = (int)pre[q];   // (m != 0 only inside the lattice)
}

// ---- fill --------------------------------------------------------------------------------------------------------------

struct Frame { float ox, oy, oz, sx, sy, sz; };

// the lattice gradient at point (i, j, k), linear index o: central differences, one-sided on a border
__device__ __forceinline__ float diff_along(const float *__restrict__ vol, size_t o, size_t stride, int p, int n, float s)
{
    const bool lo = p > 0, hi = p + 1 < n;
    const float fm = vol[lo ? o - stride : o], fp = vol[hi ? o + stride : o];
    return (fp - fm) / ((lo && hi) ? 2.0f * s : s);
}

__device__ __forceinline__ void gradient_at(const Lattice &g, const Frame &fr, const float *__restrict__ vol, size_t o, int i, int j,
                                            int k, float &gx, float &gy, float &gz)
{
    gx = diff_along(vol, o, g.sx, i, g.nx, fr.sx);
    gy = diff_along(vol, o, g.sy, j, g.ny, fr.sy);
    gz = diff_along(vol, o, 1, k, g.nz, fr.sz);
}

__global__ void __launch_bounds__(TB) iso_vertex_kernel(Lattice g, const float *__restrict__ vol, float level, Frame fr,
                                                        const unsigned char *__restrict__ mask, const int *__restrict__ base,
                                                        long long n_verts, float *__restrict__ verts, float *__restrict__ normals)
{
    // Four consecutive points per thread, their masks in one load (the mask array is 128-byte aligned): the ids are the
    // count's, so nothing ties a point to its workgroup of the other passes, and the few points with crossed edges walk
    // their dependent loads side by side in many threads instead of one after the other in one.
    const unsigned L0 = (blockIdx.x * (unsigned)TB + threadIdx.x) * 4u;
    if (L0 >= g.N) return;
    unsigned m4;
    if (L0 + 3u < g.N) m4 = *reinterpret_cast<const unsigned *>(mask + L0);
    else m4 = (unsigned)mask[L0] | (L0 + 1u < g.N ? (unsigned)mask[L0 + 1u] << 8 : 0u) | (L0 + 2u < g.N ? (unsigned)mask[L0 + 2u] << 16 : 0u);
    for (; m4 != 0u; ) {
        const int p4 = (__ffs((int)m4) - 1) >> 3;   // the next of the four points with a crossed edge
        unsigned m = (m4 >> (8 * p4)) & 0xffu;
        m4 &= ~(0xffu << (8 * p4));
        const unsigned L = L0 + (unsigned)p4;
        int i, j, k;
        unflatten(g, L, i, j, k);
        const float fa = vol[L];
        long long id = base[L];
        float gax = 0.0f, gay = 0.0f, gaz = 0.0f;
        if (normals) gradient_at(g, fr, vol, L, i, j, k, gax, gay, gaz);
        for (; m != 0u; m &= m - 1u, ++id) {
            const int c = __ffs((int)m);   // the direction code: bit c - 1
            const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
            // a code the mask should not hold (a workspace that is not the count's) reads nothing outside the volume
            if (i + dx >= g.nx || j + dy >= g.ny || k + dz >= g.nz || id < 0 || id >= n_verts) continue;
            const size_t ob = (size_t)L + (size_t)dx * g.sx + (size_t)dy * g.sy + (size_t)dz;
            const float fb = vol[ob];
            const float t = (level - fa) / (fb - fa);
            const float px = (float)i + (dx ? t : 0.0f), py = (float)j + (dy ? t : 0.0f), pz = (float)k + (dz ? t : 0.0f);
            float *v = verts + 3 * id;
            v[0] = fr.ox + px * fr.sx;
            v[1] = fr.oy + py * fr.sy;
            v[2] = fr.oz + pz * fr.sz;
            if (normals) {
                float gbx, gby, gbz;
                gradient_at(g, fr, vol, ob, i + dx, j + dy, k + dz, gbx, gby, gbz);
                const float gx = gax + t * (gbx - gax), gy = gay + t * (gby - gay), gz = gaz + t * (gbz - gaz);
                const float n = sqrtf((gx * gx + gy * gy) + gz * gz);
                const bool ok = n > 0.0f;
                float *nn = normals + 3 * id;
                nn[0] = ok ? (-gx) / n : 0.0f;
                nn[1] = ok ? (-gy) / n : 0.0f;
                nn[2] = ok ? (-gz) / n : 0.0f;
            }
        }
    }
}

// The triangles of one tetrahedron by its sign case (bit v: corner v is inside), as edges of the tetrahedron 0..5 = 01, 02,
// 03, 12, 13, 23, three bits each, for a tetrahedron whose corners are positively oriented; derivation: for one inside corner
// s and an even permutation (s, x, y, z) of the corners the triangle (sx, sy, sz) is counter-clockwise seen from outside
// (three inside: reversed); for two inside corners and an even permutation (s1, s2, o1, o2) the quad is (s1o1, s1o2, s2o2,
// s2o1), split along its first and third corner.
__device__ __forceinline__ unsigned tet_case(int m)
{
#define R2_TRI(a, b, c) ((unsigned)(a) | (unsigned)(b) << 3 | (unsigned)(c) << 6)
#define R2_CASE(n, t0, t1) ((unsigned)(n) << 18 | (t0) | (t1) << 9)
    static constexpr unsigned TABLE[16] = {
        R2_CASE(0, 0u, 0u),
        R2_CASE(1, R2_TRI(0, 1, 2), 0u),                  //  1: 0 inside
        R2_CASE(1, R2_TRI(0, 4, 3), 0u),                  //  2: 1
        R2_CASE(2, R2_TRI(1, 2, 4), R2_TRI(1, 4, 3)),     //  3: 0 1
        R2_CASE(1, R2_TRI(1, 3, 5), 0u),                  //  4: 2
        R2_CASE(2, R2_TRI(2, 0, 3), R2_TRI(2, 3, 5)),     //  5: 0 2
        R2_CASE(2, R2_TRI(0, 4, 5), R2_TRI(0, 5, 1)),     //  6: 1 2
        R2_CASE(1, R2_TRI(2, 4, 5), 0u),                  //  7: 3 outside
        R2_CASE(1, R2_TRI(2, 5, 4), 0u),                  //  8: 3
        R2_CASE(2, R2_TRI(0, 1, 5), R2_TRI(0, 5, 4)),     //  9: 0 3
        R2_CASE(2, R2_TRI(3, 0, 2), R2_TRI(3, 2, 5)),     // 10: 1 3
        R2_CASE(1, R2_TRI(1, 5, 3), 0u),                  // 11: 2 outside
        R2_CASE(2, R2_TRI(1, 3, 4), R2_TRI(1, 4, 2)),     // 12: 2 3
        R2_CASE(1, R2_TRI(0, 3, 4), 0u),                  // 13: 1 outside
        R2_CASE(1, R2_TRI(0, 2, 1), 0u),                  // 14: 0 outside
        R2_CASE(0, 0u, 0u),
    };
#undef R2_TRI
#undef R2_CASE
    return TABLE[m & 15];
}

__device__ __forceinline__ int pick6(const int (&e)[6], unsigned idx)
{
    return idx == 0u ? e[0] : idx == 1u ? e[1] : idx == 2u ? e[2] : idx == 3u ? e[3] : idx == 4u ? e[4] : e[5];
}

// The faces of tetrahedron TET of a cell.  in: the inside bits of the cell's corners; ms, bs: mask and first vertex id of the
// corners (the seven that own edges).  Every corner index is a compile-time constant, so the arrays stay in registers.
template <int TET>
__device__ __forceinline__ void emit_tet(unsigned in, const int (&ms)[8], const int (&bs)[8], long long &at, long long n_tris,
                                         int *__restrict__ faces)
{
    constexpr int C0 = tet_corner(TET, 0), C1 = tet_corner(TET, 1), C2 = tet_corner(TET, 2), C3 = tet_corner(TET, 3);
    const int m = (int)(((in >> C0) & 1u) | ((in >> C1) & 1u) << 1 | ((in >> C2) & 1u) << 2 | ((in >> C3) & 1u) << 3);
    if (m == 0 || m == 15) return;
    // the vertex on the edge from corner U to corner V (U's offsets are a subset of V's: U owns it, its code is V - U)
#define R2_EDGE(U, V) (bs[U] + (int)__popc((unsigned)ms[U] & ((1u << ((V) - (U) - 1)) - 1u)))
    const int e[6] = {R2_EDGE(C0, C1), R2_EDGE(C0, C2), R2_EDGE(C0, C3), R2_EDGE(C1, C2), R2_EDGE(C1, C3), R2_EDGE(C2, C3)};
#undef R2_EDGE
    const unsigned cs = tet_case(m);
    const int n = (int)(cs >> 18);
    for (int r = 0; r < n; ++r, ++at) {
        const unsigned tri = (cs >> (9 * r)) & 0x1ffu;
        const int a = pick6(e, tri & 7u), b = pick6(e, (tri >> 3) & 7u), c = pick6(e, (tri >> 6) & 7u);
        if (at < 0 || at >= n_tris) continue;
        int *f = faces + 3 * at;
        f[0] = a;
        f[1] = tet_mirrored(TET) ? c : b;
        f[2] = tet_mirrored(TET) ? b : c;
    }
}

__global__ void __launch_bounds__(TB) iso_face_kernel(Lattice g, const float *__restrict__ vol, float level,
                                                      const unsigned char *__restrict__ mask, const unsigned char *__restrict__ tcnt,
                                                      const int *__restrict__ base, const long long *__restrict__ off_t,
                                                      long long n_tris, int *__restrict__ faces)
{
    // Every cell's offset is the prefix of the triangle counts in point order.  Cells with triangles are few (a surface), and a
    // cell's work is a chain of dependent loads: the wave first lists its cells with triangles in LDS -- point and offset,
    // both relative to the wave's run, in point order by ballots -- and then deals the list over its lanes, so that the
    // chains of a wave run side by side whichever of its 16 rounds of points they come from.
    __shared__ unsigned list[TB / WAVE][PPW];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const unsigned first = wave_first();
    int tc[ITER];
#pragma unroll
    for (int q = 0; q < ITER; ++q) {
        const unsigned L = first + (unsigned)q * WAVE + lane;
        tc[q] = L < g.N ? (int)tcnt[L] : 0;
    }
    int run = 0, listed = 0;   // wave-uniform: triangles and listed cells of the rounds so far
#pragma unroll
    for (int q = 0; q < ITER; ++q) {
        const int incl = wave_inclusive(tc[q], lane);
        const unsigned long long active = __ballot(tc[q] != 0);
        if (tc[q] != 0)   // offset < 1024 * 12 < 2^14, point < 2^10
            list[wave][listed + __popcll(active & ((1ull << lane) - 1ull))] = (unsigned)(run + incl - tc[q]) << 10 | (unsigned)(q * WAVE + lane);
        run += __shfl(incl, WAVE - 1);
        listed += __popcll(active);
    }
    const long long wave_at = off_t[blockIdx.x] + waves_before(run);   // (the barrier inside also orders the list's writes)
    for (int e = lane; e < listed; e += WAVE) {
        const unsigned entry = list[wave][e];
        const unsigned L = first + (entry & 1023u);
        long long at = wave_at + (entry >> 10);
        int i, j, k;
        unflatten(g, L, i, j, k);
        if (i + 1 >= g.nx || j + 1 >= g.ny || k + 1 >= g.nz) continue;   // (not a cell: not from the count)
        // the cell's corners: inside bits, and the mask and first vertex of the seven that own edges of the cell
        unsigned in = 0u;
        int ms[8], bs[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t o = (size_t)L + (size_t)(u & 1) * g.sx + (size_t)((u >> 1) & 1) * g.sy + (size_t)(u >> 2);
            in |= (unsigned)(vol[o] >= level) << u;
            ms[u] = u < 7 ? (int)mask[o] : 0;
            bs[u] = u < 7 ? base[o] : 0;
        }
        emit_tet<0>(in, ms, bs, at, n_tris, faces);
        emit_tet<1>(in, ms, bs, at, n_tris, faces);
        emit_tet<2>(in, ms, bs, at, n_tris, faces);
        emit_tet<3>(in, ms, bs, at, n_tris, faces);
        emit_tet<4>(in, ms, bs, at, n_tris, faces);
        emit_tet<5>(in, ms, bs, at, n_tris, faces);
    }
}

bool lattice_refused(const char *entry, int nx, int ny, int nz, const float *vol, Lattice &g)
{
    if (nx < 1 || ny < 1 || nz < 1 || !vol) {
        set_error("%s: invalid argument (every dimension at least 1, a volume)", entry);
        return true;
    }
    const unsigned long long N = (unsigned long long)nx * (unsigned long long)ny * (unsigned long long)nz;
    if (N >= (1ull << 31)) {
        set_error("%s: %d x %d x %d lattice points, fewer than 2^31 are supported", entry, nx, ny, nz);
        return true;
    }
    g = Lattice{nx, ny, nz, (unsigned)ny * (unsigned)nz, (unsigned)nz, (unsigned)N, nx >= 2 && ny >= 2 && nz >= 2};
    return false;
}

}  // namespace

}  // namespace r2

extern "C" size_t r2_isosurface_workspace_bytes(int nx, int ny, int nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    const unsigned long long N = (unsigned long long)nx * (unsigned long long)ny * (unsigned long long)nz;
    if (N >= (1ull << 31)) return 0;
    return r2::carve(nullptr, (unsigned)N).bytes;
}

extern "C" int r2_isosurface_count(int nx, int ny, int nz, const float *vol, float level, void *ws, size_t ws_bytes,
                                   long long *counts, void *stream)
{
    using namespace r2;
    const char *entry = "r2_isosurface_count";
    Lattice g;
    if (lattice_refused(entry, nx, ny, nz, vol, g)) return R2_ERR_INVALID;
    if (!counts || !ws || ws_bytes < r2_isosurface_workspace_bytes(nx, ny, nz)) {
        set_error("%s: no counts, or a workspace of %zu bytes where r2_isosurface_workspace_bytes asks for %zu", entry,
                  ws ? ws_bytes : (size_t)0, r2_isosurface_workspace_bytes(nx, ny, nz));
        return R2_ERR_INVALID;
    }
    const Work w = carve(ws, g.N);
    const unsigned nb = blocks_of(g.N);
    hipStream_t s = (hipStream_t)stream;
    iso_count_kernel<<<dim3(nb), dim3(TB), 0, s>>>(g, vol, level, w);
    iso_scan_kernel<<<dim3(1), dim3(SCAN), 0, s>>>(nb, w, counts);
    iso_base_kernel<<<dim3(nb), dim3(TB), 0, s>>>(g, w);
    R2_STAGE_CHECK(0, s, "isosurface count");
    return 0;
}

extern "C" int r2_isosurface_fill(int nx, int ny, int nz, const float *vol, float level, float ox, float oy, float oz, float sx,
                                  float sy, float sz, const void *ws, size_t ws_bytes, long long n_verts, long long n_tris,
                                  float *verts, float *normals, int *faces, void *stream)
{
    using namespace r2;
    const char *entry = "r2_isosurface_fill";
    Lattice g;
    if (lattice_refused(entry, nx, ny, nz, vol, g)) return R2_ERR_INVALID;
    if (n_verts < 0 || n_tris < 0 || n_verts >= (1ll << 31) || n_tris >= (1ll << 31)) {
        set_error("%s: %lld vertices and %lld triangles, each must lie in [0, 2^31)", entry, n_verts, n_tris);
        return R2_ERR_INVALID;
    }
    if (!ws || ws_bytes < r2_isosurface_workspace_bytes(nx, ny, nz) || (n_verts > 0 && !verts) || (n_tris > 0 && !faces)) {
        set_error("%s: no output, or a workspace of %zu bytes where r2_isosurface_workspace_bytes asks for %zu", entry,
                  ws ? ws_bytes : (size_t)0, r2_isosurface_workspace_bytes(nx, ny, nz));
        return R2_ERR_INVALID;
    }
    if (!g.cells || (n_verts == 0 && n_tris == 0)) return 0;
    const Work w = carve(const_cast<void *>(ws), g.N);
    const unsigned nb = blocks_of(g.N);
    const Frame fr{ox, oy, oz, sx, sy, sz};
    hipStream_t s = (hipStream_t)stream;
    if (n_verts > 0) iso_vertex_kernel<<<dim3((g.N + 4 * TB - 1) / (4 * TB)), dim3(TB), 0, s>>>(g, vol, level, fr, w.mask, w.base, n_verts, verts, normals);
    if (n_tris > 0) iso_face_kernel<<<dim3(nb), dim3(TB), 0, s>>>(g, vol, level, w.mask, w.tcnt, w.base, w.off_t, n_tris, faces);
    R2_STAGE_CHECK(0, s, "isosurface fill");
    return 0;
}
