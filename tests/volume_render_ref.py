"""NumPy restatement of the direct volume renderer (csrc/volume_render.hip; include/r2hip.h: r2_volume_bricks,
r2_render_volume, r2_render_volume_mip).  Host only; the product never imports this file.

* ``walk``: the ray of every pixel, its clip, sample count and trilinear sample values in float32, operation by operation
  as csrc/ray_sampling.hpp and csrc/trilinear.hpp write them (only their explicit fmaf calls are fused: the ``_fma32``
  rule of tests/fdk_ref.py), with the brick every sample belongs to.
* ``bricks`` / ``brick_range`` / ``empty_bricks``: the min/max table and the conservative tests on it, in float32.
* ``mip``: the maximum of the sample values.  ``composite``: the compositing loop, in float32 as the kernel orders it, or in
  float64 fed the float32 sample values and dl.
* ``measure_e32(case)``: the largest |float32 - float64| over the four channels of a named case with t_stop = 0;
  ``python -m tests.volume_render_ref`` writes tests/golden/volume_render/e32.json.

The cases are the smallest that straddle the kernel's constants: a wave tile is 8 x 8 pixels, a block 16 x 16, a brick 8
cells, the table at most 1024 rows.
"""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "volume_render", "e32.json")
U = 2.0 ** -24
BRICK = 8
F32 = np.float32


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma32(a, b, c):
    """fmaf of float32 arrays by the rule of tests/fdk_ref.py's _fma32: the product is exact in float64, the sum is rounded
    once there and once to float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


# ---- the walk --------------------------------------------------------------------------------------------------------------------

def _axis_of(q, n):
    f = np.floor(np.fmin(np.fmax(q, F32(-2.0)), F32(n) + F32(1.0)))
    i = f.astype(np.int64)
    w = q - f
    w0 = np.where((i >= 0) & (i < n), F32(1.0) - w, F32(0.0)).astype(np.float32)
    w1 = np.where((i + 1 >= 0) & (i + 1 < n), w, F32(0.0)).astype(np.float32)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), w0, w1


def _trilinear(vol, X, Y, Z):
    def pair(w0, w1, a, b):
        return _fma32(w1, b, w0 * a)
    c = {}
    for ix, xi in enumerate((X[0], X[1])):
        for iy, yi in enumerate((Y[0], Y[1])):
            c[ix, iy] = pair(Z[2], Z[3], vol[xi, yi, Z[0]], vol[xi, yi, Z[1]])
    c0 = pair(Y[2], Y[3], c[0, 0], c[0, 1])
    c1 = pair(Y[2], Y[3], c[1, 0], c[1, 1])
    return pair(X[2], X[3], c0, c1)


def walk(vol, rays12, cone, H, W, dVoxel, accuracy):
    """-> dict(hit [R], n [R], dl [R] float32, f [R, nmax] float32 sample values (0 beyond n), brick [R, nmax] the linear brick
    index of every sample (-1 beyond n)), R = V H W pixels in row-major order."""
    vol = _f32(vol)
    n3 = vol.shape
    R12 = _f32(rays12)
    v, r, c = (a.ravel() for a in np.meshgrid(np.arange(len(R12)), np.arange(H), np.arange(W), indexing="ij"))
    Rv, fc, fr = R12[v], _f32(c), _f32(r)
    P = [(Rv[:, 3 + a] + fc * Rv[:, 6 + a]) + fr * Rv[:, 9 + a] for a in range(3)]
    if cone:
        s = [Rv[:, a] for a in range(3)]
        d = [P[a] - s[a] for a in range(3)]
    else:
        s, d = P, [Rv[:, a] for a in range(3)]
    t0 = np.full(len(v), 0.0 if cone else -np.inf, np.float32)
    t1 = np.full(len(v), np.inf, np.float32)
    inside = np.ones(len(v), bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            lo, hi = F32(-1.0), F32(n3[a])
            zero = d[a] == 0
            ta, tb = (lo - s[a]) / d[a], (hi - s[a]) / d[a]
            t0 = np.where(zero, t0, np.fmax(t0, np.fmin(ta, tb)))
            t1 = np.where(zero, t1, np.fmin(t1, np.fmax(ta, tb)))
            inside &= np.where(zero, (s[a] > lo) & (s[a] < hi), True)
        hit = inside & (t1 > t0)
        span = t1 - t0
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        nf = np.ceil(span * length / F32(accuracy))
        n = np.where(hit, np.maximum(1, np.fmin(np.where(hit, nf, 1), F32(2.0 ** 30)).astype(np.int64)), 0)
        dt = span / np.maximum(n, 1).astype(np.float32)
        wd = [d[a] * F32(dVoxel[a]) for a in range(3)]
        wlen = np.sqrt((wd[0] * wd[0] + wd[1] * wd[1]) + wd[2] * wd[2])
        dl = dt * wlen
    nmax = int(n.max(initial=0))
    f = np.zeros((len(v), nmax), np.float32)
    brick = np.full((len(v), nmax), -1, np.int64)
    nb = [(m + BRICK - 1) // BRICK for m in n3]
    for k in range(nmax):
        on = np.nonzero(k < n)[0]
        t = _fma32(np.full(len(on), F32(k) + F32(0.5), np.float32), dt[on], t0[on])
        A = [_axis_of(_fma32(t, d[a][on], s[a][on]), n3[a]) for a in range(3)]
        f[on, k] = _trilinear(vol, *A)
        brick[on, k] = ((A[0][0] >> 3) * nb[1] + (A[1][0] >> 3)) * nb[2] + (A[2][0] >> 3)
    return dict(hit=hit, n=n, dl=np.where(hit, dl, F32(0)).astype(np.float32), f=f, brick=brick)


# ---- the brick table -------------------------------------------------------------------------------------------------------------

def bricks(vol):
    """[bx,by,bz,2] float32: min and max over the voxels [8 b, min(8 b + 8, n - 1)] of each axis, widened to contain 0 on the
    faces of the volume, zeros stored as +0."""
    vol = _f32(vol)
    n3 = vol.shape
    nb = [(m + BRICK - 1) // BRICK for m in n3]
    out = np.zeros(tuple(nb) + (2,), np.float32)
    for i in range(nb[0]):
        for j in range(nb[1]):
            for k in range(nb[2]):
                b = (i, j, k)
                sl = tuple(slice(BRICK * b[a], min(BRICK * b[a] + BRICK, n3[a] - 1) + 1) for a in range(3))
                mn, mx = vol[sl].min(), vol[sl].max()
                if any(b[a] == 0 or BRICK * b[a] + BRICK > n3[a] - 1 for a in range(3)):
                    mn, mx = np.fmin(mn, F32(0)), np.fmax(mx, F32(0))
                out[i, j, k] = (mn + F32(0), mx + F32(0))
    return out


def brick_range(table):
    """(lo, hi) float32 of every brick: [mn - 8 u M, mx + 8 u M], rounded outwards by one float32 where M > 0."""
    mn, mx = table[..., 0], table[..., 1]
    pad = np.fmax(np.abs(mn), np.abs(mx)) * F32(8 * U)
    lo, hi = mn - pad, mx + pad
    return np.nextafter(lo, lo - pad), np.nextafter(hi, hi + pad)


def _cell(f, lo, scale, K):
    """(x, i) of values f in the table, in f's precision: fmax / fmin put a NaN on 0, as fmaxf / fminf do."""
    T = f.dtype.type
    x = np.fmin(np.fmax((f - lo) * scale, T(0)), T(K - 1))
    return x, np.minimum(np.floor(x).astype(np.int64), K - 2)


def empty_bricks(table, lut, lo, hi):
    """bool per brick: the compositing kernel's conservative test -- every row the brick's range can reach has ext == 0."""
    lut = _f32(lut)
    K = len(lut)
    lo, scale = F32(lo), F32(K - 1) / (F32(hi) - F32(lo))
    a, b = brick_range(table)
    _, ia = _cell(a, lo, scale, K)
    xb, ib = _cell(b, lo, scale, K)
    last = np.where(xb > ib.astype(np.float32), ib + 1, ib)
    nzp = np.concatenate([[0], np.cumsum(lut[:, 3] != 0)])
    return nzp[last + 1] == nzp[ia]


# ---- the two renderers -----------------------------------------------------------------------------------------------------------

def mip(w):
    """[R] float32: fmax over the samples from -inf; 0 for a ray that misses."""
    best = np.full(len(w["n"]), -np.inf, np.float32)
    for k in range(w["f"].shape[1]):
        best = np.where(k < w["n"], np.fmax(best, w["f"][:, k]), best)
    return np.where(w["hit"], best, F32(0)).astype(np.float32)


def composite(w, lut, lo, hi, t_stop=0.0, dtype=np.float32):
    """-> ([R,4] (C_r, C_g, C_b, 1 - T) in ``dtype``, [R] number of samples composited).  float32: the kernel's operations in
    its order; float64: the same formulas fed the float32 sample values, dl, lo, hi and table."""
    T = dtype
    lut = _f32(lut).astype(T)
    K = len(lut)
    lo_t, hi_t = T(F32(lo)), T(F32(hi))
    scale = T(K - 1) / (hi_t - lo_t)
    R = len(w["n"])
    C = np.zeros((R, 3), T)
    Tr = np.ones(R, T)
    dl = w["dl"].astype(T)
    stopped = np.zeros(R, bool)
    used = np.zeros(R, np.int64)
    for k in range(w["f"].shape[1]):
        on = (k < w["n"]) & ~stopped
        f = w["f"][:, k].astype(T)
        x, i = _cell(f, lo_t, scale, K)
        wt = x - i.astype(T)
        a, b = lut[i], lut[i + 1]
        ch = a + wt[:, None] * (b - a)
        e = np.exp(-(ch[:, 3] * dl))
        wgt = Tr * (T(1) - e)
        C = np.where(on[:, None], C + wgt[:, None] * ch[:, :3], C)
        Tr = np.where(on, Tr * e, Tr)
        used += on
        stopped |= on & (Tr < T(t_stop))
    out = np.concatenate([C, (T(1) - Tr)[:, None]], 1)
    assert out.dtype == T
    return np.where(w["hit"][:, None], out, T(0)), used


# ---- cameras and tables for the cases ---------------------------------------------------------------------------------------------

def camera_rays(eye, target, up, H, W, nVoxel, dVoxel, fov_y=None, ortho_height=None):
    """[1,12] float32 {a, p00, pu, pv} in voxel-index coordinates of a look-at camera over a volume centred at the world origin
    (float64, then rounded), pixel (r, c) at NDC ((2c+1)/W - 1, (2r+1)/H - 1), rows against ``up``; and cone."""
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    ez = (target - eye) / np.linalg.norm(target - eye)
    ex = np.cross(ez, up)
    ex /= np.linalg.norm(ex)
    ey = np.cross(ez, ex)
    d = np.asarray(dVoxel, np.float64)
    corner = -0.5 * d * np.asarray(nVoxel, np.float64)
    to_idx = lambda p: (p - corner) / d - 0.5   # noqa: E731
    if fov_y is not None:
        ty = np.tan(np.radians(fov_y) / 2)
        tx = ty * W / H
        a = to_idx(eye)
        p00 = to_idx(eye + ex * (1.0 / W - 1.0) * tx + ey * (1.0 / H - 1.0) * ty + ez)
    else:
        ty = ortho_height / 2
        tx = ty * W / H
        a = ez / d
        p00 = to_idx(eye + ex * (1.0 / W - 1.0) * tx + ey * (1.0 / H - 1.0) * ty)
    return np.concatenate([a, p00, ex * (2 * tx / W) / d, ey * (2 * ty / H) / d])[None].astype(np.float32), fov_y is not None


def orbit(azimuths, elevation, distance, H, W, nVoxel, dVoxel, fov_y=40.0, target=(0.0, 0.0, 0.0)):
    el = np.radians(elevation)
    eyes = [distance * np.array([np.cos(el) * np.cos(np.radians(a)), np.cos(el) * np.sin(np.radians(a)), np.sin(el)])
            for a in azimuths]
    return np.concatenate([camera_rays(e, target, (0, 0, 1), H, W, nVoxel, dVoxel, fov_y=fov_y)[0] for e in eyes], 0)


def ramp_lut(K, unit, colours=None):
    """The "linear" opacity ramp over a grey ramp (or ``colours`` [K,3]) with extinction -log1p(-min(a, 1 - 2^-24)) / unit."""
    a = np.linspace(0.0, 1.0, K)
    rgb = np.repeat(a[:, None], 3, 1) if colours is None else np.asarray(colours, np.float64)
    ext = -np.log1p(-np.minimum(a, 1.0 - 2.0 ** -24)) / unit
    return np.concatenate([rgb, ext[:, None]], 1).astype(np.float32)


def random_lut(K, seed, ext_max):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(0, 1, (K, 3)), rng.uniform(0, ext_max, (K, 1))], 1).astype(np.float32)


def _dense():
    n, dv = (9, 16, 17), (0.1, 0.12, 0.09)
    vol = np.random.RandomState(3).uniform(-0.5, 1.0, n).astype(np.float32)
    return dict(vol=vol, rays=orbit((20.0, 140.0, 260.0), 25.0, 3.0, 17, 33, n, dv), cone=True, H=17, W=33, dVoxel=dv,
                accuracy=0.5, lut=ramp_lut(256, 0.3), clim=(-0.25, 1.0))


def _inside():
    n, dv = (15, 7, 25), (0.08, 0.1, 0.05)
    vol = np.random.RandomState(4).uniform(0.0, 1.0, n).astype(np.float32)
    rays, _ = camera_rays((0.11, 0.07, -0.2), (0.6, 0.3, 0.4), (0, 0, 1), 16, 9, n, dv, fov_y=90.0)   # the source inside
    lut = np.array([[0.9, 0.1, 0.2, 0.0], [0.2, 0.8, 0.3, 2.0], [0.1, 0.3, 1.0, 5.0]], np.float32)
    return dict(vol=vol, rays=rays, cone=True, H=16, W=9, dVoxel=dv, accuracy=0.5, lut=lut, clim=(0.1, 0.9))


def _axis():
    # parallel rays along +x, two zero direction components; pixel points on integer y and z, brick faces (8, 16) among them,
    # some columns outside the support of z
    n, dv = (16, 17, 9), (0.05, 0.05, 0.05)
    vol = np.random.RandomState(5).uniform(-0.2, 1.0, n).astype(np.float32)
    rays = np.array([[1, 0, 0, -3, 2, -1, 0, 0, 1, 0, 2, 0]], np.float32)
    return dict(vol=vol, rays=rays, cone=False, H=8, W=15, dVoxel=dv, accuracy=0.5, lut=random_lut(1024, 6, 8.0), clim=(0.0, 1.0))


def _miss():
    # view 0 sees the volume in a corner of its image, view 1 looks away from it, view 2 sees it whole
    n, dv = (5, 8, 17), (0.2, 0.1, 0.06)
    vol = np.random.RandomState(7).uniform(0.0, 1.0, n).astype(np.float32)
    rays = np.concatenate([orbit((30.0,), 10.0, 2.5, 7, 1, n, dv, fov_y=30.0, target=(0.0, 0.0, 0.7)),
                           orbit((150.0,), 10.0, 2.5, 7, 1, n, dv, fov_y=30.0, target=(-5.0, 3.0, 1.0)),
                           orbit((270.0,), 10.0, 2.5, 7, 1, n, dv, fov_y=60.0)], 0)
    lut = np.array([[0.1, 0.2, 0.3, 0.0], [1.0, 0.9, 0.8, 4.0]], np.float32)
    return dict(vol=vol, rays=rays, cone=True, H=7, W=1, dVoxel=dv, accuracy=0.5, lut=lut, clim=(0.0, 1.0))


def _constant():
    n, dv = (2, 8, 8), (0.3, 0.1, 0.1)
    vol = np.full(n, 0.7, np.float32)
    rays, _ = camera_rays((1.5, -1.1, 0.8), (0, 0, 0), (0, 0, 1), 9, 8, n, dv, ortho_height=1.6)
    colours = np.random.RandomState(8).uniform(0, 1, (256, 3))
    return dict(vol=vol, rays=rays, cone=False, H=9, W=8, dVoxel=dv, accuracy=0.5, lut=ramp_lut(256, 0.2, colours), clim=(0.0, 1.0))


def _single():
    n, dv = (1, 1, 1), (0.5, 0.4, 0.3)
    vol = np.full(n, 0.9, np.float32)
    lut = np.array([[0.0, 0.0, 0.0, 0.0], [0.5, 0.4, 0.3, 1.0], [1.0, 1.0, 0.9, 3.0]], np.float32)
    return dict(vol=vol, rays=orbit((70.0,), -30.0, 2.0, 15, 7, n, dv), cone=True, H=15, W=7, dVoxel=dv, accuracy=0.5, lut=lut,
                clim=(0.0, 1.0))


def _sparse():
    # a few blobs in zeros under the "linear" ramp: most of the 4^3 bricks test empty
    n, dv = (25, 25, 25), (0.04, 0.04, 0.04)
    vol = np.zeros(n, np.float32)
    vol[2:5, 3:6, 2:4] = 0.8
    vol[18:21, 10:12, 20:23] = 0.5
    vol[7:10, 15:18, 8:9] = 0.95
    return dict(vol=vol, rays=orbit((200.0,), 20.0, 1.6, 33, 16, n, dv), cone=True, H=33, W=16, dVoxel=dv, accuracy=0.5,
                lut=ramp_lut(256, 0.1), clim=(0.0, 1.0))


KAPPA = 2.5


def _beer_lambert():
    # colour 1 and an extinction KAPPA * value over [0, 1]: alpha = 1 - exp(-KAPPA * line integral)
    n, dv = (7, 15, 8), (0.12, 0.06, 0.1)
    vol = np.random.RandomState(9).uniform(0.0, 1.0, n).astype(np.float32)
    lut = np.array([[1, 1, 1, 0.0], [1, 1, 1, KAPPA]], np.float32)
    return dict(vol=vol, rays=orbit((110.0,), 35.0, 2.2, 9, 17, n, dv), cone=True, H=9, W=17, dVoxel=dv, accuracy=0.5, lut=lut,
                clim=(0.0, 1.0))


CASES = {"beer_lambert": _beer_lambert, "dense_orbit": _dense, "inside_cone": _inside, "parallel_axis": _axis, "partial_miss": _miss, "constant": _constant,
         "single_voxel": _single, "sparse_blobs": _sparse}


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case with its walk, computed once and shared: treat every array as read-only."""
    c = CASES[name]()
    c["walk"] = walk(c["vol"], c["rays"], c["cone"], c["H"], c["W"], c["dVoxel"], c["accuracy"])
    for v in list(c.values()) + list(c["walk"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float32 [R,4], float64 [R,4]) of a case with t_stop = 0."""
    c = case(name)
    return (composite(c["walk"], c["lut"], *c["clim"], dtype=np.float32)[0],
            composite(c["walk"], c["lut"], *c["clim"], dtype=np.float64)[0])


def measure_e32(name):
    r32, r64 = reference(name)
    return float(np.abs(r32.astype(np.float64) - r64).max())


def load_e32():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    res = {n: measure_e32(n) for n in CASES}
    with open(GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    for n, v in res.items():
        print(n, "%.3e (%.1f u)" % (v, v / U))
