"""Restatement of the projection-conditioning entries (include/r2hip.h: r2_proj_resize, r2_proj_median) and of the device
steps of prepare_real.py.  Host only; the product never imports this file.

Every function takes ``dtype``.  In float32 each line is one separately rounded IEEE operation in the order the header states
(NumPy float32 arithmetic rounds each add and multiply once and never fuses): that is the kernels operation for operation.
In float64 the same statements run on the same float32 tables and weights, widened: the reference the float32 rounding is
measured against.  The median sorts its window, which shares nothing with the kernel's selection network.
"""
import numpy as np

F32 = np.float32


def prepared(src, shift=(0, 0), lo=None, dtype=F32):
    """P of the header for src [..., H, W]: the input moved by ``shift`` with zeros beyond it, values below ``lo`` raised to it."""
    src = np.asarray(src, dtype=F32)
    H, W = src.shape[-2:]
    sr, sc = shift
    out = np.zeros(src.shape, dtype=F32)
    r = np.arange(H) + sr
    c = np.arange(W) + sc
    rin, cin = (r >= 0) & (r < H), (c >= 0) & (c < W)
    if rin.any() and cin.any():
        x = src[..., r[rin][:, None], c[cin][None, :]]
        if lo is not None:
            x = np.where(x < F32(lo), F32(lo), x)
        out[..., np.nonzero(rin)[0][:, None], np.nonzero(cin)[0][None, :]] = x
    return out.astype(dtype)


def linear_table(n, m):
    """-> (s [m] int, f [m] float32): the header's taps and fractions of an axis with n inputs and m outputs."""
    inv = float(m) / float(n)
    scale = 1.0 / inv
    d = np.arange(m, dtype=np.float64)
    fx = ((d + 0.5) * scale - 0.5).astype(F32)
    fl = np.floor(fx)
    s = fl.astype(np.int64)
    f = fx - fl                                  # float32
    low, high = s < 0, s >= n - 1
    s = np.where(low, 0, np.where(high, n - 1, s))
    f = np.where(low | high, F32(0), f).astype(F32)
    return s, f


def _window(size, crop):
    mh, mw = size
    return (0, 0, mh, mw) if crop is None else tuple(int(v) for v in crop)


def resize_linear(src, size, shift=(0, 0), lo=None, crop=None, dtype=F32):
    """r2_proj_resize with interp = 0 on src [..., H, W] -> [..., oh, ow]."""
    P = prepared(src, shift, lo, dtype)
    H, W = P.shape[-2:]
    r0, c0, oh, ow = _window(size, crop)
    sy, fy = linear_table(H, size[0])
    sx, fx = linear_table(W, size[1])
    sy, fy, sx, fx = sy[r0:r0 + oh], fy[r0:r0 + oh], sx[c0:c0 + ow], fx[c0:c0 + ow]
    ra, rb = sy[:, None], np.minimum(sy + 1, H - 1)[:, None]
    ca, cb = sx[None, :], np.minimum(sx + 1, W - 1)[None, :]
    b1, b0 = fy[:, None].astype(dtype), (F32(1) - fy)[:, None].astype(dtype)     # 1.f - f is a float32 operation
    a1, a0 = fx[None, :].astype(dtype), (F32(1) - fx)[None, :].astype(dtype)
    with np.errstate(invalid="ignore"):
        h0 = P[..., ra, ca] * a0 + P[..., ra, cb] * a1
        h1 = P[..., rb, ca] * a0 + P[..., rb, cb] * a1
        return h0 * b0 + h1 * b1


def resize_area(src, size, shift=(0, 0), lo=None, crop=None, dtype=F32):
    """r2_proj_resize with interp = 1: the block's sum row after row, then times (float)(1 / (fy fx))."""
    P = prepared(src, shift, lo, dtype)
    H, W = P.shape[-2:]
    mh, mw = size
    assert H % mh == 0 and W % mw == 0
    fy, fx = H // mh, W // mw
    r0, c0, oh, ow = _window(size, crop)
    blk = P.reshape(P.shape[:-2] + (mh, fy, mw, fx))[..., r0:r0 + oh, :, c0:c0 + ow, :]
    acc = blk[..., :, 0, :, 0].copy()
    with np.errstate(invalid="ignore"):
        for i in range(fy):
            for j in range(fx):
                if i or j:
                    acc = acc + blk[..., :, i, :, j]
        return acc * dtype(F32(1.0 / (fy * fx)))


def median(src, k, dtype=F32):
    """r2_proj_median's m for src [..., H, W]: rank k k / 2 of the replicated-border window, a NaN read as +inf."""
    x = np.asarray(src, dtype=dtype)
    x = np.where(np.isnan(x), dtype(np.inf), x)
    r = k // 2
    H, W = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)], mode="edge")
    win = np.stack([p[..., i:i + H, j:j + W] for i in range(k) for j in range(k)], axis=-1)
    return np.ascontiguousarray(np.sort(win, axis=-1)[..., k * k // 2])


def despeckle(src, k, threshold, dtype=F32):
    """-> (dst, replace) of r2_proj_median with conditional = 1."""
    x = np.asarray(src, dtype=dtype)
    m = median(x, k, dtype)
    with np.errstate(invalid="ignore"):
        replace = ~(np.abs(x - m) <= dtype(threshold))
    return np.where(replace, m, x), replace


# ---- prepare_real.py's steps ---------------------------------------------------------------------------------------------------

def host_scale(img, proj_rescale, object_scale):
    return (np.asarray(img) / proj_rescale * object_scale).astype(F32)


def square_window(mh, mw):
    """The window the reference's slices leave of an mh x mw image, found by slicing an image of pixel numbers."""
    idx = np.arange(mh * mw).reshape(mh, mw)
    if mh > mw:
        off = int((mh - mw) / 2)
        idx = idx[off:-off, :]
    elif mh < mw:
        off = int((mw - mh) / 2)
        idx = idx[:, off:-off]
    if idx.size == 0:
        return None
    return int(idx[0, 0] // mw), int(idx[0, 0] % mw), idx.shape[0], idx.shape[1]


def real_projection(img, proj_rescale=400.0, object_scale=50, subsample=4, despeckle_threshold=None, k=3):
    """One projection of prepare_real.py in float32 (subsample != 1)."""
    p = host_scale(img, proj_rescale, object_scale)
    if despeckle_threshold is not None:
        p = despeckle(p, k, despeckle_threshold)[0]
    mh, mw = int(p.shape[0] / subsample), int(p.shape[1] / subsample)
    return resize_linear(p, (mh, mw), shift=(5, 0), lo=0.0, crop=square_window(mh, mw))


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------------

# (H, W) -> (mh, mw): single pixels and lines, an upscale that takes the s < 0 branch, integer and non-integer factors
RESIZE_SHAPES = [((1, 1), (1, 1)), ((1, 7), (3, 2)), ((5, 1), (2, 4)), ((6, 5), (13, 11)), ((8, 12), (2, 3)),
                 ((37, 300), (9, 70)), ((70, 1000), (17, 333))]
AREA_CASES = [((8, 12), (4, 4)), ((5, 9), (1, 3)), ((6, 7), (2, 1))]          # (H, W), (fy, fx)
MEDIAN_SHAPES = [(1, 1), (2, 9), (7, 1), (2, 2), (9, 11), (33, 70)]


def case_stack(V, shape, seed=0):
    """Normal data around 0.3, a third of it negative; float32, no exact zeros."""
    rng = np.random.RandomState(3000 + seed + 7 * shape[0] + 13 * shape[1] + V)
    x = (rng.randn(V, *shape) * 0.7 + 0.3).astype(F32)
    x[x == 0] = F32(0.5)
    return x
