"""Per-pixel weights of the training projections: detector defect masks, the fill of unmeasured pixels for the FDK
initialisation, and the trainer's ``--loss_weights`` modes.  Plain numpy (and ``uncertainty.noise_weights``); the weights
themselves are consumed by ``losses.image_loss(..., weights=)`` and ``uncertainty.fisher_diagonal(..., weights=)``.

A weight counts only where it is > 0; a pixel of weight 0 is unmeasured and its value in the projection is never used (a case
written by ``datagen`` holds 0 there, so that readers which ignore the weights stay finite; NaN is as good).  A case records
one static detector mask ``weights_train.npy`` [H, W], shared by all training views; [V, H, W] is read as well.
"""
import numpy as np

MODES = ("auto", "none", "file", "noise")


def defect_mask(nDetector, rng, dead_pixels=0.0, dead_lines=0, gap=None):
    """A static detector mask [H, W], float32, 1 = measured, 0 = not, for ``nDetector`` = (H, W).  ``dead_pixels``: the fraction
    of the detector's pixels that are dead singly, round(fraction H W) distinct ones; ``dead_lines``: the number of whole dead
    rows or columns, distinct lines drawn from the H rows and W columns alike; ``gap`` = (c0, c1): the columns c0 <= c < c1 (a
    gap between two panels).  Deterministic in ``rng`` (a numpy RandomState or Generator), which is drawn from only for the
    defects asked for: first the pixels, then the lines."""
    H, W = int(nDetector[0]), int(nDetector[1])
    if H < 1 or W < 1:
        raise ValueError("nDetector must be (H, W) with H, W >= 1, got %r" % (tuple(nDetector),))
    if not 0.0 <= float(dead_pixels) <= 1.0:
        raise ValueError("dead_pixels is a fraction in [0, 1], got %r" % (dead_pixels,))
    if int(dead_lines) != dead_lines or not 0 <= int(dead_lines) <= H + W:
        raise ValueError("dead_lines must be an integer in [0, %d], got %r" % (H + W, dead_lines))
    mask = np.ones((H, W), np.float32)
    n_pix = int(round(float(dead_pixels) * H * W))
    if n_pix > 0:
        mask.reshape(-1)[rng.choice(H * W, size=n_pix, replace=False)] = 0.0
    if int(dead_lines) > 0:
        for line in rng.choice(H + W, size=int(dead_lines), replace=False):
            if line < H:
                mask[int(line), :] = 0.0
            else:
                mask[:, int(line) - H] = 0.0
    if gap is not None:
        c0, c1 = int(gap[0]), int(gap[1])
        if not 0 <= c0 < c1 <= W:
            raise ValueError("gap must be (c0, c1) with 0 <= c0 < c1 <= %d, got %r" % (W, tuple(gap)))
        mask[:, c0:c1] = 0.0
    return mask


def _per_view(weights, shape):
    """[H, W] or [V, H, W] weights against a [V, H, W] stack -> the counted weights broadcast to the stack (float32)."""
    w = np.asarray(weights, np.float32)
    if w.shape != tuple(shape[-2:]) and w.shape != tuple(shape):
        raise ValueError("weights are %s but the projections are %s" % (w.shape, tuple(shape)))
    with np.errstate(invalid="ignore"):
        w = np.where(w > 0, w, np.float32(0))
    return np.broadcast_to(w, shape)


def fill_unmeasured(projs, weights, radius=2):
    """``projs`` ([V, H, W] or [H, W]) with every unmeasured pixel (weight not > 0) replaced by the mean of the measured pixels
    of its (2 radius + 1)^2 window, 0 where the window has none; measured pixels are returned bit for bit.  float32.  What an
    unmeasured pixel holds (0, NaN, anything) does not enter.  For consumers that cannot take weights: the FDK initialisation."""
    p = np.asarray(projs, np.float32)
    if p.ndim not in (2, 3):
        raise ValueError("projs must be [V, H, W] or [H, W], got %s" % (p.shape,))
    radius = int(radius)
    if radius < 0:
        raise ValueError("radius must be >= 0, got %d" % radius)
    stack = p[None] if p.ndim == 2 else p
    m = _per_view(weights, stack.shape) > 0
    V, H, W = stack.shape
    val = np.zeros((V, H + 2 * radius, W + 2 * radius), np.float64)
    cnt = np.zeros_like(val)
    val[:, radius:radius + H, radius:radius + W] = np.where(m, stack, 0.0)
    cnt[:, radius:radius + H, radius:radius + W] = m
    s, c = np.zeros((V, H, W)), np.zeros((V, H, W))
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            s += val[:, dy:dy + H, dx:dx + W]
            c += cnt[:, dy:dy + H, dx:dx + W]
    fill = np.where(c > 0, s / np.maximum(c, 1.0), 0.0).astype(np.float32)
    out = np.where(m, stack, fill)
    return out[0] if p.ndim == 2 else out


def resolve_weights(case, mode):
    """The training weights of a case as ``recon._read_case`` returns it, for the trainer's ``--loss_weights`` ``mode``:
    ``auto``: the case's recorded ``weights_train`` if it has any, else None; ``none``: None; ``file``: the recorded weights, a
    ValueError without; ``noise``: ``uncertainty.noise_weights`` of the raw training stack (before the scene scale) under the
    scanner config's ``possion_noise`` and ``gaussian_noise``, times the recorded weights if there are any (the stack's
    unmeasured pixels do not enter).  -> None, or float32 [H, W] / [V, H, W] with every weight that does not count set to 0."""
    if mode not in MODES:
        raise ValueError("loss weights mode must be one of %s, got %r" % (", ".join(MODES), mode))
    recorded = case.get("weights_train")
    if mode == "none" or (mode == "auto" and recorded is None):
        return None
    projs = case["train"][0]
    if mode == "file" and recorded is None:
        raise ValueError("--loss_weights file: the case records no weights_train")
    if mode in ("auto", "file"):
        w = np.asarray(recorded, np.float32)
        _per_view(w, projs.shape)
        with np.errstate(invalid="ignore"):
            return np.where(w > 0, w, np.float32(0))
    from .uncertainty import noise_weights
    cfg = case["cfg"]
    if "possion_noise" not in cfg or "gaussian_noise" not in cfg:
        raise ValueError("--loss_weights noise: the scanner config has no possion_noise / gaussian_noise")
    if recorded is None:
        return noise_weights(projs, cfg["possion_noise"], cfg["gaussian_noise"])
    m = _per_view(recorded, projs.shape)
    nw = noise_weights(np.where(m > 0, projs, np.float32(0)), cfg["possion_noise"], cfg["gaussian_noise"])
    return np.where(m > 0, nw * m, np.float32(0)).astype(np.float32)
