"""Helpers of tests/test_fdk_edges_{cpu,gpu}.py: the cases that put the FDK back-projection (csrc/fdk.hip) at its launch
edges and detector borders, a float32 restatement of the kernel's chain that can carry planted mistakes, and the error
unit both tests measure in.

The unit.  The detector coordinate of a voxel is a float32 of magnitude W (or H); its rounding moves a bilinear sample by
at most twice the largest |q| of the 4 x 4 pixels around the footprint, per pixel of displacement.  So an error is measured
in units of  eps32 * (W + H + 8) * T,  T = sum over the views of  weight * (largest |q| in that neighbourhood, counting
zero outside the detector).  Unlike the interpolated sample the neighbourhood maximum does not cancel, and it stays non-zero
while a footprint is within a pixel of the border, where a correct float32 chain may legitimately round to the other side.
K = 8 units is the acceptance of the GPU kernel; the restatement itself stays under K / 4, a half-pixel shift or a
clamped border is beyond 10 K (tests/test_fdk_edges_cpu.py asserts all three)."""
import functools

import numpy as np

from oracle import fdk_oracle as F
from r2_gaussian_amd import scene as S

K = 8.0
EPS32 = float(np.finfo(np.float32).eps)
DSO = 5.0
ANGLES = (0.0, 0.37, np.pi / 2, 2.9, 4.1, 5.9)
DETECTORS = ((7, 5), (20, 33), (64, 96))   # (H, W)
# nVoxel, sVoxel, centre -- what each one exercises is in the names
VOLUMES = {
    "1x1x1-smallest-launch": ((1, 1, 1), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0)),
    "3x7x70-ny%4=3-nz=64+6": ((3, 7, 70), (3.2, 3.0, 3.4), (0.1, -0.2, 0.05)),
    "2x17x64-ny=16+1-nz=one-wave": ((2, 17, 64), (2.0, 1.6, 2.2), (0.05, -0.1, 0.02)),
    "5x16x65-one-lane-past-a-wave-off-detector": ((5, 16, 65), (6.0, 6.0, 6.0), (0.0, 0.0, 0.0)),
    "4x3x129-ny<BY-three-z-blocks": ((4, 3, 129), (2.0, 2.0, 7.0), (0.0, 0.0, 0.0)),
}
# the volumes that reach past the detector of both beams (the cone beam's detector sees +-1.43 at the axis, the parallel +-1)
PAST_THE_DETECTOR = ("3x7x70-ny%4=3-nz=64+6", "5x16x65-one-lane-past-a-wave-off-detector", "4x3x129-ny<BY-three-z-blocks")
assert set(PAST_THE_DETECTOR) <= set(VOLUMES)
CASES = [(vol, det, cone) for vol in VOLUMES for det in DETECTORS for cone in (True, False)]


def case_id(case):
    vol, (H, W), cone = case
    return "%s-det%dx%d-%s" % (vol, H, W, "cone" if cone else "parallel")


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma32(a, b, c):
    """fmaf of float32 operands: the product is exact in float64, the sum is rounded once there and once to float32."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def backproject_f32(q, full_proj, DSO, nVoxel, sVoxel, center, cone=True, shift_fx=0.0, clamp_border=False):
    """fdk_backproject_kernel and its launcher restated in numpy float32, operation by operation (only the explicit fmaf
    calls are fused).  q [V,H,W], full_proj [V,4,4] -> vol [nx,ny,nz] float32.
    Planted mistakes: ``shift_fx`` is added to the pixel coordinate fx (0.5: a half-pixel convention slip),
    ``clamp_border`` returns the nearest detector pixel where the kernel's taps return zero."""
    q = _f32(q)
    V, H, W = q.shape
    nx, ny, nz = (int(n) for n in nVoxel)
    one, half = np.float32(1.0), np.float32(0.5)
    s = [np.float32(v) for v in sVoxel]
    c = [np.float32(v) for v in center]
    d = [s[k] / np.float32(n) for k, n in enumerate((nx, ny, nz))]
    o = [(c[k] - half * s[k]) + half * d[k] for k in range(3)]
    X = (o[0] + _f32(np.arange(nx)) * d[0])[:, None, None]
    Y = (o[1] + _f32(np.arange(ny)) * d[1])[None, :, None]
    Z = (o[2] + _f32(np.arange(nz)) * d[2])[None, None, :]
    hW, hH = half * np.float32(W), half * np.float32(H)
    dso = np.float32(DSO)
    acc = np.zeros((nx, ny, nz), np.float32)
    for v in range(V):
        M = _f32(full_proj[v]).reshape(16)
        bx = (X * M[0] + Z * M[8]) + M[12]
        by = (X * M[1] + Z * M[9]) + M[13]
        bw = (X * M[3] + Z * M[11]) + M[15]
        hx, hy, hw = _fma32(Y, M[4], bx), _fma32(Y, M[5], by), _fma32(Y, M[7], bw)
        inv = one / (hw + np.float32(0.0000001))
        fx = (hx * inv + one) * hW - half + np.float32(shift_fx)
        fy = (hy * inv + one) * hH - half
        flx, fly = np.floor(fx), np.floor(fy)
        ax, ay = fx - flx, fy - fly
        u0 = np.minimum(np.maximum(flx, np.float32(-2.0)), np.float32(W)).astype(np.int64)
        v0 = np.minimum(np.maximum(fly, np.float32(-2.0)), np.float32(H)).astype(np.int64)

        def tap(u, w):
            ok = (u >= 0) & (u < W) & (w >= 0) & (w < H)
            x = q[v][np.clip(w, 0, H - 1), np.clip(u, 0, W - 1)]
            return x if clamp_border else np.where(ok, x, np.float32(0.0))

        s00, s01, s10, s11 = tap(u0, v0), tap(u0 + 1, v0), tap(u0, v0 + 1), tap(u0 + 1, v0 + 1)
        smp = (one - ay) * ((one - ax) * s00 + ax * s01) + ay * ((one - ax) * s10 + ax * s11)
        wi = dso * inv
        acc = acc + (smp * (wi * wi) if cone else smp)
    return acc


def tap_bound(q, full_proj, DSO, nVoxel, sVoxel, center, cone=True, return_stats=False):
    """T [nx,ny,nz] float64 (see the module's docstring), from the oracle's footprints.  With ``return_stats`` also a dict
    of what the footprints do at the detector's borders:
      inside    [nx,ny,nz] bool: all four bilinear taps are detector pixels in every view
      straddle  {"u<0", "u>=W", "v<0", "v>=H"} -> bool: in some view some voxel's four taps lie across that border (some on
                the detector, the others past that border)
      min_hw    the smallest homogeneous w (the distance in front of the source for a cone beam)"""
    qa = np.abs(np.asarray(q, dtype=np.float64))
    V, H, W = qa.shape
    P = 4
    T = np.zeros([int(n) for n in nVoxel])
    inside = np.ones(T.shape, bool)
    straddle = {"u<0": False, "u>=W": False, "v<0": False, "v>=H": False}
    min_hw = np.inf
    for v, (fx, fy, inv) in enumerate(F.voxel_footprints(full_proj[:V], H, W, nVoxel, sVoxel, center)):
        x0 = np.floor(fx)
        y0 = np.floor(fy)
        pad = np.zeros((H + 2 * P, W + 2 * P))
        pad[P:P + H, P:P + W] = qa[v]
        # beyond [-3, n + 1] the whole neighbourhood [x0 - 1, x0 + 2] is off the detector: clipping there keeps it so
        xi = np.clip(x0, -3, W + 1).astype(np.int64) + P
        yi = np.clip(y0, -3, H + 1).astype(np.int64) + P
        N = np.zeros(T.shape)
        for dy in (-1, 0, 1, 2):
            for dx in (-1, 0, 1, 2):
                N = np.maximum(N, pad[yi + dy, xi + dx])
        T += ((DSO * inv) ** 2 if cone else 1.0) * N
        u_in, v_in = (x0 >= 0) & (x0 <= W - 2), (y0 >= 0) & (y0 <= H - 2)
        inside &= u_in & v_in
        u_some, v_some = (x0 >= -1) & (x0 <= W - 1), (y0 >= -1) & (y0 <= H - 1)
        straddle["u<0"] |= bool(((x0 == -1) & v_some).any())
        straddle["u>=W"] |= bool(((x0 == W - 1) & v_some).any())
        straddle["v<0"] |= bool(((y0 == -1) & u_some).any())
        straddle["v>=H"] |= bool(((y0 == H - 1) & u_some).any())
        min_hw = min(min_hw, float((1.0 / inv).min()))
    if return_stats:
        return T, dict(inside=inside, straddle=straddle, min_hw=min_hw)
    return T


def unit(T, H, W):
    """One unit of error per voxel."""
    return EPS32 * (W + H + 8) * T


def worst_ratio(got, ref, T, H, W):
    """max over the voxels with T > 0 of |got - ref| in units (0 when there is none)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    m = T > 0
    return float((err[m] / unit(T[m], H, W)).max()) if m.any() else 0.0


@functools.lru_cache(maxsize=None)
def scene(case):
    """Everything a case's tests share, computed once and left unchanged: the views' matrices, the filtered projections q
    (uniform in [-0.5, 0.5]), the oracle's volume, T and the border statistics."""
    vol, (H, W), cone = case
    n, s, ctr = VOLUMES[vol]
    scanner = S.CONE_BEAM if cone else S.PARALLEL_BEAM
    fp = np.stack([S.make_view(a, (H, W), scanner).full_proj_transform.numpy() for a in ANGLES])
    rng = np.random.RandomState(1000 * H + W + (7 if cone else 0) + 13 * n[2])
    q = (rng.rand(len(ANGLES), H, W) - 0.5).astype(np.float32)
    ref = F.fdk_backproject(q, fp, DSO, n, s, ctr, cone)
    T, stats = tap_bound(q, fp, DSO, n, s, ctr, cone, return_stats=True)
    for a in (fp, q, ref, T, stats["inside"]):
        a.setflags(write=False)
    return dict(H=H, W=W, cone=cone, n=n, s=s, ctr=ctr, fp=fp, q=q, ref=ref, T=T, stats=stats)
