"""GPU: the weighted image loss (r2_loss_l1_ssim_weighted[_batch] of csrc/loss_ops.hip through the C ABI and through
losses.image_loss / image_loss_batch with ``weights=``).

* Against the float64 restatement of tests/weighted_loss_ref.py: every gradient element and the scalars within the derived
  float32 bounds (that file states how each follows from the kernels' roundings), at the shapes where tiled kernels go wrong
  and with weight patterns that empty single pixels, a whole tile, a band of columns or everything.  Margins (error / bound)
  go to PARITY_LOG.
* Bit identities that need no tolerance: no weights and unit weights are the unweighted kernels; a power-of-two scale of
  the weights changes nothing; what an unmeasured pixel's measurement holds changes nothing; negative and NaN weights are
  zeros; two runs agree; the batched call is the single-view call per view.
* The C ABI writes nothing outside dL_dimg, the scratch of exactly *_scratch_floats and the scalars.
"""
import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import weighted_loss_ref as WR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 37), (37, 1), (5, 7), (11, 11), (16, 16), (15, 17), (17, 15), (33, 31), (127, 129)]
PATTERNS = ["ones", "rand", "mask", "one_pixel", "tile_off", "column_gap", "all_zero"]
LAM = 0.25


def _images(hw, seed=0):
    rng = np.random.default_rng(hw[0] * 7919 + hw[1] * 31 + seed)
    gt = rng.random(hw, dtype=np.float32)
    img = np.clip(gt + 0.1 * rng.standard_normal(hw, dtype=np.float32), 0, None).astype(np.float32)
    return img, gt


def _weights(hw, pattern, seed=0):
    """-> float32 [H, W], or None where the shape has no such pattern (tile_off needs a whole 16 x 16 tile)."""
    H, W = hw
    rng = np.random.default_rng(H * 104729 + W * 17 + seed)
    rand = (2.0 * (1.0 - rng.random(hw))).astype(np.float32)                 # (0, 2]
    if pattern == "ones":
        return np.ones(hw, np.float32)
    if pattern == "rand":
        return rand
    if pattern == "mask":
        return (rand * (rng.random(hw) > 0.3)).astype(np.float32)
    if pattern == "one_pixel":
        w = np.zeros(hw, np.float32)
        w[H // 2, W // 2] = 0.7
        return w
    if pattern == "tile_off":
        if H < 16 or W < 16:
            return None
        w = rand.copy()
        w[:16, :16] = 0
        return w
    if pattern == "column_gap":
        w = rand.copy()
        w[:, W // 3:W // 3 + max(1, W // 8)] = 0
        return w
    assert pattern == "all_zero"
    return np.zeros(hw, np.float32)


def _nan_under_zeros(gt, w):
    out = gt.copy()
    out[~(w > 0)] = np.nan
    return out


def _margin(err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, np.where(bound > 0, err / bound, np.inf))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------- the C ABI, raw
SENTINEL = 0x7FC0FFEE       # a NaN bit pattern no kernel writes
GUARD = 64                  # floats each side (keeps 256-byte alignment of the sub-range)


def _guarded(n, dev):
    buf = torch.empty(n + 2 * GUARD, dtype=torch.float32, device=dev)
    buf.view(torch.int32).fill_(SENTINEL)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    w = buf.view(torch.int32).cpu().numpy()
    return bool((w[:GUARD] == SENTINEL).all() and (w[GUARD + n:] == SENTINEL).all())


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _raw_weighted(img, gt, w, dev, w_l1=1.0, w_ssim=LAM):
    """r2_loss_l1_ssim_weighted on guarded sub-ranges -> (grad [H, W], scalars [4]) host arrays, after asserting every guard
    word and that every gradient element and scalar was written.  w None: NULL."""
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd._C import _stream
    L = _lib.lib()
    H, W = img.shape
    x, y, wt = _dev(img, dev), _dev(gt, dev), _dev(w, dev)
    ns = int(L.r2_loss_l1_ssim_weighted_scratch_floats(W, H))
    bg, g = _guarded(H * W, dev)
    bs, s = _guarded(ns, dev)
    bc, c = _guarded(4, dev)
    rc = L.r2_loss_l1_ssim_weighted(W, H, x.data_ptr(), y.data_ptr(), None if wt is None else wt.data_ptr(), float(w_l1),
                                    float(w_ssim), g.data_ptr(), s.data_ptr(), c.data_ptr(), _stream(dev))
    _lib.check(rc, "r2_loss_l1_ssim_weighted")
    torch.cuda.synchronize()
    for buf, n, what in ((bg, H * W, "dL_dimg"), (bs, ns, "scratch"), (bc, 4, "scalars")):
        assert _guards_intact(buf, n), "r2_loss_l1_ssim_weighted %dx%d wrote outside %s" % (H, W, what)
    assert not (g.view(torch.int32).cpu().numpy() == SENTINEL).any(), "a gradient element was not written"
    assert not (c.view(torch.int32).cpu().numpy() == SENTINEL).any(), "a scalar was not written"
    return g.cpu().numpy().reshape(H, W), c.cpu().numpy()


def _raw_unweighted(img, gt, dev, w_l1=1.0, w_ssim=LAM):
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd._C import _stream
    L = _lib.lib()
    H, W = img.shape
    x, y = _dev(img, dev), _dev(gt, dev)
    g = torch.empty(H, W, device=dev)
    s = torch.empty(int(L.r2_loss_l1_ssim_scratch_floats(W, H)), device=dev)
    c = torch.empty(3, device=dev)
    _lib.check(L.r2_loss_l1_ssim(W, H, x.data_ptr(), y.data_ptr(), float(w_l1), float(w_ssim), g.data_ptr(), s.data_ptr(),
                                 c.data_ptr(), _stream(dev)), "r2_loss_l1_ssim")
    torch.cuda.synchronize()
    return g.cpu().numpy(), c.cpu().numpy()


def _raw_weighted_batch(imgs, gts, ws, dev, w_l1=1.0, w_ssim=LAM, table=True):
    """r2_loss_l1_ssim_weighted_batch on guarded sub-ranges -> (grad [V, H, W], scalars [V + 1, 4]).  ws: a list of arrays and
    None entries; table False passes weights_host = NULL."""
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd._boundary import ptr_table
    from r2_gaussian_amd._C import _stream
    L = _lib.lib()
    V, H, W = imgs.shape
    x = _dev(imgs, dev)
    ys, wts = [_dev(g, dev) for g in gts], [_dev(w, dev) for w in ws]
    ns = int(L.r2_loss_l1_ssim_weighted_batch_scratch_floats(V, W, H))
    bg, g = _guarded(V * H * W, dev)
    bs, s = _guarded(ns, dev)
    bc, c = _guarded(4 * (V + 1), dev)
    rc = L.r2_loss_l1_ssim_weighted_batch(V, W, H, x.data_ptr(), ptr_table(ys), ptr_table(wts) if table else None, float(w_l1),
                                          float(w_ssim), g.data_ptr(), s.data_ptr(), c.data_ptr(), _stream(dev))
    _lib.check(rc, "r2_loss_l1_ssim_weighted_batch")
    torch.cuda.synchronize()
    for buf, n, what in ((bg, V * H * W, "dL_dimg"), (bs, ns, "scratch"), (bc, 4 * (V + 1), "scalars")):
        assert _guards_intact(buf, n), "r2_loss_l1_ssim_weighted_batch %dx%dx%d wrote outside %s" % (V, H, W, what)
    assert not (g.view(torch.int32).cpu().numpy() == SENTINEL).any(), "a gradient element was not written"
    assert not (c.view(torch.int32).cpu().numpy() == SENTINEL).any(), "a scalar was not written"
    return g.cpu().numpy().reshape(V, H, W), c.cpu().numpy().reshape(V + 1, 4)


# ------------------------------------------------------------------------------------------------- against float64
def _check_against_float64(hw, pattern, gpu):
    from r2_gaussian_amd.losses import image_loss
    w = _weights(hw, pattern)
    if w is None:
        return
    img, gt = _images(hw)
    gt_used = _nan_under_zeros(gt, w)                       # the unmeasured measurements are NaN throughout
    ref = WR.weighted_l1_ssim64(img, gt_used, w, 1.0, LAM)
    b = WR.weighted_bounds(ref)
    assert b["cond_ok"], "the content leaves first-order error propagation (B2 error >= B2 / 2): not a valid case"
    a = torch.from_numpy(img).to(gpu).requires_grad_(True)
    loss, parts = image_loss(a, torch.from_numpy(gt_used).to(gpu), LAM, weights=torch.from_numpy(w).to(gpu))
    loss.backward()
    torch.cuda.synchronize()
    got = a.grad.cpu().numpy().astype(np.float64)
    p = parts.cpu().numpy().astype(np.float64)
    assert p.shape == (4,) and float(loss.detach()) == p[2]
    err = np.abs(got - ref["grad"])
    stats = dict(kind="loss_l1_ssim_weighted", case="%dx%d_%s" % (hw[0], hw[1], pattern),
                 grad_margin=float(_margin(err, b["grad"]).max()), l1_margin=float(_margin(abs(p[0] - ref["l1"]), b["l1"])),
                 ssim_margin=float(_margin(abs(p[1] - ref["ssim"]), b["ssim"])),
                 loss_margin=float(_margin(abs(p[2] - ref["loss"]), b["loss"])),
                 sum_w_margin=float(_margin(abs(p[3] - ref["sum_w"]), b["sum_w"])))
    Hh.PARITY_LOG.append(stats)
    print(stats)
    assert np.isfinite(got).all() and np.isfinite(p).all(), stats
    assert (err <= b["grad"]).all(), (stats, np.unravel_index(np.argmax(_margin(err, b["grad"])), err.shape))
    assert max(stats["l1_margin"], stats["ssim_margin"], stats["loss_margin"], stats["sum_w_margin"]) <= 1.0, (stats, p)
    if pattern == "all_zero" or not (w > 0).any():
        assert p.tolist() == [0.0, 1.0, 0.0, 0.0] and not got.any()


@pytest.mark.parametrize("hw", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_weighted_loss_against_float64(hw, gpu):
    for pattern in PATTERNS:
        _check_against_float64(hw, pattern, gpu)


def test_weighted_loss_fold_at_512(gpu):
    """1024 per-block sums per scalar, sum w among them."""
    _check_against_float64((512, 512), "mask", gpu)


# -------------------------------------------------------------------------------------------------- bit identities
IDENTITY_SHAPES = [(1, 1), (15, 17), (33, 31), (127, 129)]


@pytest.mark.parametrize("hw", IDENTITY_SHAPES, ids=["%dx%d" % s for s in IDENTITY_SHAPES])
def test_no_weights_and_unit_weights_are_the_unweighted_kernels(hw, gpu):
    from r2_gaussian_amd.losses import image_loss
    img, gt = _images(hw)
    g0, c0 = _raw_unweighted(img, gt, gpu)
    for w in (None, np.ones(hw, np.float32)):
        g, c = _raw_weighted(img, gt, w, gpu)
        assert np.array_equal(_bits(g), _bits(g0)) and np.array_equal(_bits(c[:3]), _bits(c0))
        assert c[3] == hw[0] * hw[1]
    # the wrapper without weights is the call it was: three scalars, the same bits
    a = torch.from_numpy(img).to(gpu).requires_grad_(True)
    loss, parts = image_loss(a, torch.from_numpy(gt).to(gpu), LAM)
    loss.backward()
    loss1, parts1 = image_loss(torch.from_numpy(img).to(gpu), torch.from_numpy(gt).to(gpu), LAM, weights=None)
    torch.cuda.synchronize()
    assert parts.shape == (3,) and parts1.shape == (3,)
    assert np.array_equal(_bits(parts.cpu().numpy()), _bits(c0)) and np.array_equal(_bits(parts1.cpu().numpy()), _bits(c0))
    assert np.array_equal(_bits(a.grad.cpu().numpy()), _bits(g0))


@pytest.mark.parametrize("hw", IDENTITY_SHAPES, ids=["%dx%d" % s for s in IDENTITY_SHAPES])
def test_weight_rules_change_no_bit(hw, gpu):
    img, gt = _images(hw)
    for pattern in ("mask", "column_gap"):
        w = _weights(hw, pattern)
        g0, c0 = _raw_weighted(img, gt, w, gpu)
        # two runs
        g, c = _raw_weighted(img, gt, w, gpu)
        assert np.array_equal(_bits(g), _bits(g0)) and np.array_equal(_bits(c), _bits(c0))
        # a power-of-two scale of the weights: the same gradient and {l1, ssim, loss}; sum w scales
        for k in (10, -10):
            g, c = _raw_weighted(img, gt, w * np.float32(2.0 ** k), gpu)
            assert np.array_equal(_bits(g), _bits(g0)) and np.array_equal(_bits(c[:3]), _bits(c0[:3])), k
            assert c[3] == np.float32(c0[3] * np.float32(2.0 ** k))
        # what an unmeasured pixel's measurement holds
        for fill in (np.nan, np.inf, 1e30):
            other = gt.copy()
            other[~(w > 0)] = fill
            g, c = _raw_weighted(img, other, w, gpu)
            assert np.array_equal(_bits(g), _bits(g0)) and np.array_equal(_bits(c), _bits(c0)), fill
        # negative and NaN weights in the place of zeros
        bad = w.copy()
        zeros = np.argwhere(~(w > 0))
        for n, (i, j) in enumerate(zeros):
            bad[i, j] = (-1.5, np.nan, -np.inf, -0.0)[n % 4]
        g, c = _raw_weighted(img, gt, bad, gpu)
        assert np.array_equal(_bits(g), _bits(g0)) and np.array_equal(_bits(c), _bits(c0))
        assert np.isfinite(g0).all() and np.isfinite(c0).all()


@pytest.mark.parametrize("hw", IDENTITY_SHAPES, ids=["%dx%d" % s for s in IDENTITY_SHAPES])
def test_no_measured_pixel_gives_zero_loss_and_zero_gradient(hw, gpu):
    img, gt = _images(hw)
    for w in (np.zeros(hw, np.float32), np.full(hw, np.nan, np.float32), np.full(hw, -1.0, np.float32)):
        g, c = _raw_weighted(img, np.full(hw, np.nan, np.float32), w, gpu)
        assert c.tolist() == [0.0, 1.0, 0.0, 0.0]
        assert not g.any() and np.isfinite(g).all()


# ------------------------------------------------------------------------------------------------------- the batch
def _batch_case(V, hw, seed=3):
    """V views; the weights cycle through None, all-zero, mask, rand, column_gap (NaN measurements under the zeros)."""
    imgs, gts, ws = [], [], []
    for v in range(V):
        img, gt = _images(hw, seed=seed + v)
        w = [None, _weights(hw, "all_zero"), _weights(hw, "mask", v), _weights(hw, "rand", v), _weights(hw, "column_gap", v)][v % 5]
        imgs.append(img)
        gts.append(gt if w is None else _nan_under_zeros(gt, w))
        ws.append(w)
    return np.stack(imgs), gts, ws


@pytest.mark.parametrize("V", [1, 3, 16, 17])
def test_batch_is_the_single_view_call_per_view(V, gpu):
    hw = (33, 31)
    if V == 1:
        imgs, gts, ws = _batch_case(3, hw)
        imgs, gts, ws = imgs[2:], gts[2:], ws[2:]          # the masked view
    else:
        imgs, gts, ws = _batch_case(V, hw)
        assert any(w is None for w in ws) and any(w is not None and not w.any() for w in ws)
    grad, rows = _raw_weighted_batch(imgs, gts, ws, gpu)
    gw_l1, gw_ssim = float(np.float32(1.0) / np.float32(V)), float(np.float32(LAM) / np.float32(V))
    for v in range(V):
        _g, c = _raw_weighted(imgs[v], gts[v], ws[v], gpu)
        assert np.array_equal(_bits(rows[v]), _bits(c)), v
        g, _c = _raw_weighted(imgs[v], gts[v], ws[v], gpu, gw_l1, gw_ssim)
        assert np.array_equal(_bits(grad[v]), _bits(g)), v
        if ws[v] is not None and not ws[v].any():
            assert rows[v].tolist() == [0.0, 1.0, 0.0, 0.0] and not grad[v].any()
    want = [0.0, 0.0, 0.0, 0.0]
    for v in range(V):                                      # in view order, in double
        for k in range(4):
            want[k] += float(rows[v, k])
    want = [np.float32(want[0] / V), np.float32(want[1] / V), np.float32(want[2] / V), np.float32(want[3])]
    assert np.array_equal(_bits(rows[V]), _bits(np.array(want, np.float32))), (rows[V], want)
    assert np.isfinite(grad).all() and np.isfinite(rows).all()


def test_batch_without_a_weight_table_is_the_unweighted_batch(gpu):
    from r2_gaussian_amd.losses import image_loss_batch
    hw, V = (15, 17), 3
    imgs, gts, _ws = _batch_case(V, hw)
    gts = [_images(hw, seed=3 + v)[1] for v in range(V)]
    grad, rows = _raw_weighted_batch(imgs, gts, [None] * V, gpu, table=False)
    grad1, rows1 = _raw_weighted_batch(imgs, gts, [None] * V, gpu, table=True)
    assert np.array_equal(_bits(grad), _bits(grad1)) and np.array_equal(_bits(rows), _bits(rows1))
    a = torch.from_numpy(imgs).to(gpu).requires_grad_(True)
    loss, parts = image_loss_batch(a, [torch.from_numpy(g).to(gpu) for g in gts], LAM)
    loss.backward()
    torch.cuda.synchronize()
    assert parts.shape == (V + 1, 3)
    assert np.array_equal(_bits(parts.cpu().numpy()), _bits(rows[:, :3])) and np.array_equal(_bits(a.grad.cpu().numpy()), _bits(grad))
    assert (rows[:V, 3] == hw[0] * hw[1]).all() and rows[V, 3] == V * hw[0] * hw[1]


def test_batch_rejects_invalid_arguments(gpu):
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd._boundary import ptr_table
    L = _lib.lib()
    x = torch.zeros(2, 37, 53, device=gpu)
    g, c = torch.zeros_like(x), torch.zeros(3, 4, device=gpu)
    s = torch.empty(int(L.r2_loss_l1_ssim_weighted_batch_scratch_floats(2, 53, 37)), device=gpu)
    for V, W, H, table in ((0, 53, 37, ptr_table([x[0], x[1]])), (2, 0, 37, ptr_table([x[0], x[1]])),
                           (2, 53, 37, ptr_table([x[0], None])), (2, 53, 37, None)):
        rc = L.r2_loss_l1_ssim_weighted_batch(V, W, H, x.data_ptr(), table, None, 1.0, LAM, g.data_ptr(), s.data_ptr(),
                                              c.data_ptr(), None)
        assert rc == _lib.R2_ERR_INVALID and b"r2_loss_l1_ssim_weighted_batch" in L.r2_last_error()
    assert L.r2_loss_l1_ssim_weighted_batch_scratch_floats(0, 53, 37) == 0
    assert L.r2_loss_l1_ssim_weighted_scratch_floats(0, 37) == 0
    rc = L.r2_loss_l1_ssim_weighted(53, 37, x.data_ptr(), None, None, 1.0, LAM, g.data_ptr(), s.data_ptr(), c.data_ptr(), None)
    assert rc == _lib.R2_ERR_INVALID and b"r2_loss_l1_ssim_weighted" in L.r2_last_error()


# ----------------------------------------------------------------------------------------------------- the guards
GUARD_SHAPES = [(1, 1), (15, 17), (33, 31), (16, 4096)]


@pytest.mark.parametrize("hw", GUARD_SHAPES, ids=["%dx%d" % s for s in GUARD_SHAPES])
def test_abi_writes_stay_inside_their_buffers(hw, gpu):
    """_raw_weighted and _raw_weighted_batch assert the guard words around dL_dimg, the scratch and the scalars."""
    img, gt = _images(hw)
    w = _weights(hw, "mask")
    ref = WR.weighted_l1_ssim64(img, gt, w, 1.0, LAM)
    b = WR.weighted_bounds(ref)
    g, c = _raw_weighted(img, _nan_under_zeros(gt, w), w, gpu)
    assert (np.abs(g - ref["grad"]) <= b["grad"]).all() and abs(c[2] - ref["loss"]) <= b["loss"]
    imgs, gts, ws = _batch_case(3, hw)
    grad, rows = _raw_weighted_batch(imgs, gts, ws, gpu)
    assert np.isfinite(grad).all() and np.isfinite(rows).all()


# ---------------------------------------------------------------------------------------------------- the wrappers
def _loss_and_grad(image, gt, weights, lam=LAM):
    from r2_gaussian_amd.losses import image_loss
    a = image.detach().clone().requires_grad_(True)
    loss, parts = image_loss(a, gt, lam, weights=weights)
    loss.backward()
    torch.cuda.synchronize()
    return parts.cpu(), a.grad


def test_wrapper_weight_layouts_and_dtypes(gpu):
    hw = (37, 53)
    img, gt = _images(hw)
    w = _weights(hw, "mask")
    x, y, wt = torch.from_numpy(img).to(gpu), torch.from_numpy(_nan_under_zeros(gt, w)).to(gpu), torch.from_numpy(w).to(gpu)
    bits = lambda t: t.detach().float().cpu().view(torch.int32)
    p0, g0 = _loss_and_grad(x, y, wt)
    assert p0.shape == (4,) and g0.shape == hw
    for other in (wt[None], wt.cpu(), wt.double(), wt.t().contiguous().t(), wt.clone().requires_grad_(True)):
        p1, g1 = _loss_and_grad(x, y, other)
        assert torch.equal(p1.view(torch.int32), p0.view(torch.int32)) and torch.equal(bits(g1), bits(g0))
    wide = torch.zeros(37, 3, 53, device=gpu)
    wide[:, 1] = wt
    p1, g1 = _loss_and_grad(x[None], y[None], wide[:, 1])
    assert g1.shape == (1,) + hw and torch.equal(p1.view(torch.int32), p0.view(torch.int32)) and torch.equal(bits(g1[0]), bits(g0))
    # a bool mask is the 0 / 1 float mask
    mask = wt > 0
    pm, gm = _loss_and_grad(x, y, mask.float())
    for other in (mask, mask.cpu(), mask[None], mask.to(torch.uint8)):
        p1, g1 = _loss_and_grad(x, y, other)
        assert torch.equal(p1.view(torch.int32), pm.view(torch.int32)) and torch.equal(bits(g1), bits(gm))
    assert float(pm[3]) == float(mask.sum())
    # float64 / bfloat16 images: computed on the float32 values, the gradient comes back in the input's dtype
    p1, g1 = _loss_and_grad(x.double(), y, wt)
    assert g1.dtype == torch.float64 and torch.equal(p1.view(torch.int32), p0.view(torch.int32)) and torch.equal(bits(g1), bits(g0))
    xb = x.bfloat16()
    pb, gb = _loss_and_grad(xb, y, wt)
    pr, gr = _loss_and_grad(xb.float(), y, wt)
    assert gb.dtype == torch.bfloat16 and torch.equal(pb.view(torch.int32), pr.view(torch.int32))
    assert torch.equal(gb.cpu(), gr.bfloat16().cpu())
    # the weights are never differentiated
    wl = wt.clone().requires_grad_(True)
    a = x.clone().requires_grad_(True)
    from r2_gaussian_amd.losses import image_loss
    image_loss(a, y, LAM, weights=wl)[0].backward()
    assert wl.grad is None and a.grad is not None


def test_wrapper_batch_weight_forms(gpu):
    from r2_gaussian_amd.losses import image_loss_batch
    hw, V = (33, 31), 5
    imgs, gts, ws = _batch_case(V, hw)
    grad0, rows0 = _raw_weighted_batch(imgs, gts, ws, gpu)
    x = torch.from_numpy(imgs).to(gpu)
    ys = [torch.from_numpy(g).to(gpu) for g in gts]

    def run(weights, images=x):
        a = images.detach().clone().requires_grad_(True)
        loss, parts = image_loss_batch(a, ys, LAM, weights=weights)
        loss.backward()
        torch.cuda.synchronize()
        assert float(loss.detach()) == float(parts[V, 2])
        return parts.cpu().numpy(), a.grad
    # a sequence with None entries; tensors on the host, in double, [1, H, W]
    seq = [None if w is None else torch.from_numpy(w).to(gpu) for w in ws]
    for weights in (seq, tuple(seq), [None if t is None else (t.cpu(), t.double(), t[None])[k % 3] for k, t in enumerate(seq)]):
        parts, grad = run(weights)
        assert parts.shape == (V + 1, 4)
        assert np.array_equal(_bits(parts), _bits(rows0)) and np.array_equal(_bits(grad.cpu().numpy()), _bits(grad0))
    # one [V, H, W] tensor: None becomes ones
    full = torch.stack([torch.ones(hw, device=gpu) if t is None else t for t in seq])
    parts, grad = run(full)
    assert np.array_equal(_bits(parts), _bits(rows0)) and np.array_equal(_bits(grad.cpu().numpy()), _bits(grad0))
    parts, grad = run(full, x.double())
    assert grad.dtype == torch.float64 and np.array_equal(_bits(grad.float().cpu().numpy()), _bits(grad0))


def test_weighted_loss_used_twice_in_one_graph(gpu):
    from r2_gaussian_amd.losses import image_loss
    hw = (40, 48)
    img, gt = _images(hw)
    _, gt2 = _images(hw, seed=5)
    w1, w2 = _weights(hw, "mask"), _weights(hw, "column_gap")
    x = torch.from_numpy(img).to(gpu)
    y, y2 = torch.from_numpy(gt).to(gpu), torch.from_numpy(gt2).to(gpu)
    t1, t2 = torch.from_numpy(w1).to(gpu), torch.from_numpy(w2).to(gpu)
    a = x.clone().requires_grad_(True)
    l1, _ = image_loss(a, y, 0.25, weights=t1)
    l2, _ = image_loss(a, y2, 1.0, weights=t2)
    (l1 + 0.5 * l2).backward()
    _, g1 = _loss_and_grad(x, y, t1, 0.25)
    _, g2 = _loss_and_grad(x, y2, t2, 1.0)
    torch.cuda.synchronize()
    want = g1.double() + 0.5 * g2.double()
    assert (torch.abs(a.grad.double() - want) <= WR.U * (torch.abs(g1.double()) + torch.abs(0.5 * g2.double())) * 2).all()
