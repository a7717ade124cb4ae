"""Restatement of the cubic-spline resampling entries (include/r2hip.h: r2_spline_prefilter, r2_spline_zoom,
r2_spline_sample) and of resample.py's helpers.  Host only; the product never imports this file.

Every function takes ``dtype``.  In float32 each line is one separately rounded IEEE operation in the order the header states
(NumPy float32 arithmetic rounds each add, multiply and divide once and never fuses), with the header's truncated start sum:
that is the kernels operation for operation.  In float64 the start sum is scipy's exact half-sample-symmetric one and the
sampler's weights are double: that is scipy.ndimage's definition for ``order=3, mode="nearest", prefilter=True,
grid_mode=False``, the reference the float32 error is measured against.
"""
import numpy as np

PAD = 12                              # scipy's edge padding for mode="nearest"
HORIZON = 16                          # terms of the float32 start sum (R2_SPLINE_HORIZON)
POLE = np.sqrt(3.0) - 2.0
GAIN = (1.0 - POLE) * (1.0 - 1.0 / POLE)
ANTI = POLE / (POLE - 1.0)


def pad_edge(vol):
    return np.pad(vol, PAD, mode="edge")


def filter_axis(c, axis, dtype):
    """One pass of the header's line filter along ``axis`` of the padded block (a new array)."""
    c = np.moveaxis(np.array(c, dtype=dtype), axis, 0)
    n = c.shape[0]
    assert n >= 2 * PAD + 1
    z, gain, anti = dtype(POLE), dtype(GAIN), dtype(ANTI)
    c = gain * c
    if dtype == np.float32:
        s = c[0].copy()
        for i in range(1, HORIZON + 1):
            s = s + dtype(POLE ** i) * c[i]
        c[0] = c[0] + z * s
    else:
        zn, zi = POLE ** n, POLE
        s = c[0] + zn * c[n - 1]
        for i in range(1, n):
            s = s + zi * (c[i] + zn * c[n - 1 - i])
            zi *= POLE
        c[0] = c[0] + s * POLE / (1.0 - zn * zn)
    for i in range(1, n):
        c[i] = c[i] + z * c[i - 1]
    c[n - 1] = c[n - 1] * anti
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return np.ascontiguousarray(np.moveaxis(c, 0, axis))


def prefilter(vol, dtype=np.float64):
    """-> the coefficients [nx+24][ny+24][nz+24]: edge padding, then the line filter along x, y, z."""
    c = pad_edge(np.asarray(vol, dtype=dtype))
    for axis in range(3):
        c = filter_axis(c, axis, dtype)
    return c


def weights(t):
    """The four cubic B-spline weights of the fraction t, in t's precision and the header's order."""
    one, two, three, four, six = (t.dtype.type(v) for v in (1, 2, 3, 4, 6))
    w1 = (t * t * (t - two) * three + four) / six
    u = one - t
    w2 = (u * u * (u - two) * three + four) / six
    w0 = u * u * u / six
    w3 = one - w0 - w1 - w2
    return [w0, w1, w2, w3]


def zoom_table(n, m, dtype):
    """-> (start [m] int, weights [4][m] dtype): computed in double, each weight rounded to dtype once."""
    o = np.arange(m, dtype=np.float64)
    f = (n - 1) / (m - 1) if m > 1 else 1.0
    cc = o * f + PAD
    fl = np.floor(cc)
    return fl.astype(np.int64) - 1, [w.astype(dtype) for w in weights(cc - fl)]


def out_shape(shape, zoom):
    zoom = [zoom] * 3 if np.ndim(zoom) == 0 else list(zoom)
    return tuple(int(round(n * f)) for n, f in zip(shape, zoom))


def zoom_coeffs(c, shape, out, dtype=np.float64):
    """out(a,b,c) = sum_i wx_i (sum_j wy_j (sum_k wz_k coeffs(sx+i, sy+j, sz+k))), each sum left to right."""
    c = np.asarray(c, dtype=dtype)
    for axis in (2, 1, 0):
        start, w = zoom_table(shape[axis], out[axis], dtype)
        c = np.moveaxis(c, axis, -1)
        acc = w[0] * c[..., start]
        for k in range(1, 4):
            acc = acc + w[k] * c[..., start + k]
        c = np.moveaxis(acc, -1, axis)
    return np.ascontiguousarray(c)


def zoom(vol, factor, dtype=np.float64):
    """scipy.ndimage.zoom(vol, factor, mode="nearest")."""
    vol = np.asarray(vol)
    return zoom_coeffs(prefilter(vol, dtype), vol.shape, out_shape(vol.shape, factor), dtype)


def zoom_to(vol, out, dtype=np.float64):
    vol = np.asarray(vol)
    return zoom_coeffs(prefilter(vol, dtype), vol.shape, tuple(out), dtype)


def sample_coeffs(c, shape, points, dtype=np.float64):
    """scipy.ndimage.map_coordinates(order=3, mode="nearest") from the coefficients; points [N,3] in index coordinates of the
    unpadded volume.  A non-finite coordinate gives NaN."""
    c = np.asarray(c, dtype=dtype)
    p = np.asarray(points, dtype=dtype).reshape(-1, 3)
    bad = ~np.isfinite(p).all(axis=1)
    idx, ws = [], []
    for a in range(3):
        hi = dtype(shape[a] + 2 * PAD)
        x = np.where(bad, dtype(0), p[:, a]) + dtype(PAD)
        x = np.minimum(np.maximum(x, dtype(-1)), hi)
        fl = np.floor(x)
        start = fl.astype(np.int64) - 1
        tap = start[:, None] + np.arange(4)[None, :]
        last = shape[a] + 2 * PAD - 1
        idx.append(np.clip(tap, 0, last))
        ws.append(weights(x - fl))
    taps = c[idx[0][:, :, None, None], idx[1][:, None, :, None], idx[2][:, None, None, :]]   # [N,4,4,4]
    acc = None
    for i in range(4):
        inner = None
        for j in range(4):
            line = ws[2][0] * taps[:, i, j, 0]
            for k in range(1, 4):
                line = line + ws[2][k] * taps[:, i, j, k]
            inner = ws[1][j] * line if inner is None else inner + ws[1][j] * line
        acc = ws[0][i] * inner if acc is None else acc + ws[0][i] * inner
    if acc is None:
        acc = np.zeros((0,), dtype)
    acc = np.array(acc, dtype=dtype)
    acc[bad] = np.nan
    return acc


def map_coordinates(vol, points, dtype=np.float64):
    vol = np.asarray(vol)
    return sample_coeffs(prefilter(vol, dtype), vol.shape, points, dtype)


# ---- the reference's helpers (data_generator/synthetic_dataset/process_raw_data.py), on this file's zoom ----------------------

def resample(image, spacing, new_spacing=(1, 1, 1), zoom_fn=zoom):
    """``zoom_fn(volume, factors)`` does the resampling: this file's zoom, or scipy's for the fixtures."""
    spacing = np.array(list(spacing), dtype=np.float64)
    new_spacing = np.array(list(new_spacing), dtype=np.float64)
    new_shape = np.round(image.shape * (spacing / new_spacing))
    real = new_shape / image.shape
    return zoom_fn(image, real), spacing / real


def resize(scan, target_size, zoom_fn=zoom):
    f = tuple(target_size / s for s in scan.shape)
    return zoom_fn(scan, f) if any(v != 1.0 for v in f) else scan


def expand_to_cube(a):
    m = max(a.shape)
    pad = [(m - s) // 2 for s in a.shape]
    return np.pad(a, [(p, m - s - p) for p, s in zip(pad, a.shape)], mode="constant", constant_values=0)


def crop_to_cube(a):
    m = min(a.shape)
    s = [(d - m) // 2 for d in a.shape]
    return a[s[0]:s[0] + m, s[1]:s[1] + m, s[2]:s[2] + m]


def reshape_vol(image, spacing, target_size, mode=None, zoom_fn=zoom):
    if mode is not None:
        image, _ = resample(image, spacing, (1, 1, 1), zoom_fn)
        if mode == "crop":
            image = crop_to_cube(image)
        elif mode == "expand":
            image = expand_to_cube(image)
        else:
            raise ValueError("Unsupported reshape mode!")
    return resize(image, target_size, zoom_fn)


def zoom32(vol, factor):
    return zoom(np.asarray(vol, np.float32), factor, np.float32)


# ---- the cases the fixtures (tests/golden/resample) and the tests share -------------------------------------------------------

# per shape: factors above 1, below 1, non-integer, and with an output dimension of 1
ZOOM_CASES = [
    ((1, 1, 1), [3.0, 0.6, (2.5, 1.0, 3.4)]),
    ((2, 3, 1), [2.0, (0.5, 0.4, 1.0), (1.7, 2.4, 3.3)]),
    ((7, 5, 9), [1.7, (0.5, 0.61, 0.4), (0.1, 2.0, 0.15), 1.0]),
    ((13, 4, 6), [(2.3, 0.3, 1.5), 0.5, 1.21]),
    ((20, 17, 33), [0.37, (1.5, 0.3, 0.4), (0.05, 1.2, 0.61)]),
]
SAMPLE_SHAPES = [(6, 5, 7), (2, 3, 1)]
# volume shape, spacing, target size: unequal spacing, odd differences for the padding split and the crop offsets
RESHAPE_CASES = [((9, 6, 11), (1.3, 0.8, 1.1), 8, mode) for mode in (None, "crop", "expand")]


def case_volume(shape):
    """U[0,1) in float32."""
    return np.random.RandomState(1000 + sum(shape) + 7 * shape[0]).rand(*shape).astype(np.float32)


def case_points(shape, n_random=300):
    """float32 points for the sampler: random ones in and around the volume, every lattice node with a ring of one, the ends
    of the padded block (-12 and n + 11) exactly, and points beyond them."""
    n = np.array(shape, dtype=np.float64)
    rng = np.random.RandomState(2000 + sum(shape))
    rand = rng.rand(n_random, 3) * (n + 36) - 18
    lat = np.stack(np.meshgrid(*[np.arange(-1, k + 1) for k in shape], indexing="ij"), -1).reshape(-1, 3)
    edge = [[-12, -12, -12], list(n + 11), [-12, 0.5, n[2] + 11], [-13, -13, -13], list(n + 12), [-12.5, 1.25, n[2] + 11.5],
            [-12.999, 0, n[2] + 11.999], [-40, 0.3, n[2] + 40], [-1e6, 1e6, 0.25], [0, 0, 0], list(n - 1)]
    return np.concatenate([rand, lat, np.array(edge, dtype=np.float64)]).astype(np.float32)


def factor_id(f):
    return "x".join("%g" % v for v in ([f] * 3 if np.ndim(f) == 0 else f))


# The float32 restatement against scipy's float64 fixtures: the largest absolute error over every case above (zoom, sampler
# and reshape_vol chains on U[0,1) data) was measured as 5.13e-7, on a sampler point.  The tests assert four times that; the
# margin is for data other than uniform.  It bounds the rounding model, and through the bit-for-bit tests the kernels.
F32_MEASURED = 5.13e-7
F32_BOUND = 4 * F32_MEASURED
