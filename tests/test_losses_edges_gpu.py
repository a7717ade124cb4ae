"""The fused loss kernels (csrc/loss_ops.hip through r2_gaussian_amd/losses.py) against the float64 restatement of
tests/loss_ref.py at the shapes and contents where tiled kernels go wrong: images smaller than the 11-tap window or the 16-px
tile, odd pixel counts (the float2 partials after the three derivative maps), grids one tile thick, 2048^2 (the fold of 16 384
per-block sums) and 256^3 TV volumes (65 536 partials).  Every element is checked against its derived float32 bound
(loss_ref.py states how each follows from the kernels' rounding), and, as a second check, the kernel's worst error may not
exceed 4x the worst error of the float32 torch restatement (tests/mini_trainer.py, CPU) plus a few roundings of the
element's scale.  Margins (error / bound) go to PARITY_LOG (tests/conftest.py writes them out at session end).

Also: the C ABI writes nothing outside dL_dimg / dL_dvol, the scratch of exactly *_scratch_floats and the scalars (guard words
around each, in the same allocation); two calls give the same bits; the wrapper's shapes, strides and dtypes; the loss's SSIM
part equals metrics.slice_metrics on the same image."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import loss_ref as R
from tests import mini_trainer as T

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (1, 37), (37, 1), (5, 7), (11, 11), (16, 16), (15, 17), (17, 15), (33, 31), (127, 129), (256, 256)]
LARGE = [(512, 512), (1024, 1024), (2048, 2048), (16, 4096), (4096, 16)]
CONTENTS = ["rand", "equal", "zeros", "const", "blob", "large", "ties"]
SECONDARY = 4.0
UPSTREAM = 1.5


def _images(hw, kind, seed=0):
    H, W = hw
    rng = np.random.default_rng(H * 7919 + W * 31 + seed)
    gt = rng.random(hw, dtype=np.float32)
    img = np.clip(gt + 0.1 * rng.standard_normal(hw, dtype=np.float32), 0, None).astype(np.float32)
    if kind == "equal":
        img = gt.copy()
    elif kind == "zeros":
        img, gt = np.zeros(hw, np.float32), np.zeros(hw, np.float32)
    elif kind == "const":
        img, gt = np.full(hw, 0.75, np.float32), np.full(hw, 0.5, np.float32)
    elif kind == "blob":                      # a projection with air around it: exact zeros outside a bright blob
        yy, xx = np.mgrid[:H, :W].astype(np.float64)
        s2 = 2 * (max(H, W) / 6.0) ** 2
        gt = 2.0 * np.exp(-((yy - 0.45 * H) ** 2 + (xx - 0.55 * W) ** 2) / s2)
        gt = np.where(gt < 1e-3, 0.0, gt).astype(np.float32)
        img = (gt * (1.0 + 0.05 * rng.standard_normal(hw))).clip(0).astype(np.float32)
    elif kind == "large":
        gt, img = gt * 50, img * 50
    elif kind == "ties":
        img[: max(1, H // 3), : max(1, W // 3)] = gt[: max(1, H // 3), : max(1, W // 3)]
    return img, gt


def _f32_reference(img, gt, lam):
    a = torch.from_numpy(img)[None].clone().requires_grad_(True)
    b = torch.from_numpy(gt)[None]
    s = T.ssim(a, b)
    l1 = (a - b).abs().mean()
    loss = l1 + lam * (1.0 - s)
    loss.backward()
    return dict(loss=float(loss), l1=float(l1), ssim=float(s), grad=a.grad[0].numpy().astype(np.float64))


def _margin(err, bound):
    """err / bound, with 0 / 0 = 0 (an exact result where the bound is 0) and x / 0 = inf."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, np.where(bound > 0, err / bound, np.inf))


def _check_l1_ssim(hw, kind, lam, gpu):
    from r2_gaussian_amd.losses import image_loss
    img, gt = _images(hw, kind)
    r = R.l1_ssim64(img, gt, 1.0, lam)
    b = R.l1_ssim_bounds(r)
    assert b["cond_ok"], "the content leaves first-order error propagation (B2 error >= B2 / 2): not a valid case"
    a = torch.from_numpy(img).to(gpu).requires_grad_(True)
    loss, parts = image_loss(a, torch.from_numpy(gt).to(gpu), lam)
    (loss * UPSTREAM).backward()
    torch.cuda.synchronize()
    got = a.grad.cpu().numpy().astype(np.float64) / UPSTREAM
    p = parts.cpu().numpy().astype(np.float64)
    err = np.abs(got - r["grad"])
    gbound = b["grad"] + R.U * np.abs(got)          # + the rounding of grad * upstream
    stats = dict(kind="loss_l1_ssim", case="%dx%d_%s_lam%g" % (hw[0], hw[1], kind, lam),
                 grad_margin=float(_margin(err, gbound).max()), l1_margin=float(_margin(abs(p[0] - r["l1"]), b["l1"])),
                 ssim_margin=float(_margin(abs(p[1] - r["ssim"]), b["ssim"])),
                 loss_margin=float(_margin(abs(p[2] - r["loss"]), b["loss"])))
    f = _f32_reference(img, gt, lam)
    # floor: the kernel's final combination (N_OP roundings of its magnitude scale); where the exact gradient cancels to 0
    # (img == gt) the float32 restatement can come out exactly 0 while the kernel's differently ordered sum cannot
    floor = R.N_OP * R.U * float(np.max(lam / img.size * b["G"] + 1.0 / img.size))
    stats["grad_err_vs_f32_err"] = float(err.max() / (np.abs(f["grad"] - r["grad"]).max() + floor))
    Hh.PARITY_LOG.append(stats)
    assert np.isfinite(got).all() and np.isfinite(p).all()
    assert (err <= gbound).all(), (stats, np.unravel_index(np.argmax(_margin(err, gbound)), err.shape))
    assert stats["l1_margin"] <= 1.0 and stats["ssim_margin"] <= 1.0 and stats["loss_margin"] <= 1.0, stats
    # the secondary check: no worse than the float32 restatement, up to SECONDARY and the floor
    assert err.max() <= SECONDARY * np.abs(f["grad"] - r["grad"]).max() + floor, stats
    sfloor = R.N_BLOCK * R.U * np.abs(r["S"]).mean()
    assert abs(p[1] - r["ssim"]) <= SECONDARY * abs(f["ssim"] - r["ssim"]) + sfloor, (stats, p[1], f["ssim"], r["ssim"])
    assert abs(p[0] - r["l1"]) <= SECONDARY * abs(f["l1"] - r["l1"]) + (R.N_BLOCK + 1) * R.U * r["l1"], stats
    if kind in ("equal", "zeros"):
        assert p[0] == 0.0
    if kind == "zeros":
        assert p[1] == 1.0 and not got.any()


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("hw", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_l1_ssim_small_against_float64(hw, kind, gpu):
    for lam in (0.0, 0.25, 1.0):
        _check_l1_ssim(hw, kind, lam, gpu)


@pytest.mark.parametrize("kind", ["rand", "blob", "ties"])
@pytest.mark.parametrize("hw", LARGE, ids=["%dx%d" % s for s in LARGE])
def test_l1_ssim_large_against_float64(hw, kind, gpu):
    _check_l1_ssim(hw, kind, 0.25, gpu)


# ------------------------------------------------------------------------------------------------------------ TV
TV_SHAPES = [(1, 1, 1), (1, 1, 4), (2, 1, 1), (1, 17, 33), (33, 1, 65), (5, 7, 6), (6, 7, 5), (32, 32, 32), (64, 64, 64),
             (256, 256, 256)]


def _volume(shape, kind):
    rng = np.random.default_rng(int(np.prod(shape)) + len(kind))
    v = rng.random(shape, dtype=np.float32)
    if kind == "const":
        v = np.full(shape, 0.625, np.float32)
    elif kind == "integer":
        v = np.floor(v * 4).astype(np.float32)
    elif kind == "large":
        v = v * 1e4
    return v


@pytest.mark.parametrize("kind", ["rand", "const", "integer", "large"])
@pytest.mark.parametrize("shape", TV_SHAPES, ids=["x".join(map(str, s)) for s in TV_SHAPES])
def test_tv3d_against_float64(shape, kind, gpu):
    from r2_gaussian_amd.losses import tv_3d_loss
    vol = _volume(shape, kind)
    ref, grad, total, cnt = R.tv3d64(vol)
    b = R.tv3d_bounds(vol, total, cnt, grad)
    v = torch.from_numpy(vol).to(gpu).requires_grad_(True)
    tv = tv_3d_loss(v)
    (0.05 * tv).backward()
    torch.cuda.synchronize()
    up = float(np.float32(0.05))
    got = v.grad.cpu().numpy().astype(np.float64) / up
    val = float(tv)
    err = np.abs(got - grad)
    gb = b["grad"] + R.U * np.abs(got)
    stats = dict(kind="loss_tv3d", case="%s_%s" % ("x".join(map(str, shape)), kind), grad_margin=float(_margin(err, gb).max()))
    if cnt == 0:
        assert math.isnan(val) and not got.any() and np.isfinite(got).all()
        Hh.PARITY_LOG.append(stats)
        return
    stats["tv_margin"] = float(_margin(abs(val - ref), b["tv"]))
    f = T.tv3d_mean(torch.from_numpy(vol))
    stats["tv_err_vs_f32_err"] = abs(val - ref) / (abs(float(f) - ref) + R.U * ref) if ref > 0 else 0.0
    Hh.PARITY_LOG.append(stats)
    assert (err <= gb).all(), stats
    assert stats["tv_margin"] <= 1.0, (stats, val, ref)
    assert abs(val - ref) <= SECONDARY * abs(float(f) - ref) + R.U * ref, stats
    if kind == "const":
        assert val == 0.0 and not got.any()


# ------------------------------------------------------------------------------------ the C ABI: guards and folds
SENTINEL = 0x7FC0FFEE       # a NaN bit pattern no kernel writes
GUARD = 64                  # floats each side (keeps 256-byte alignment of the sub-range)


def _guarded(n, dev):
    buf = torch.empty(n + 2 * GUARD, dtype=torch.float32, device=dev)
    buf.view(torch.int32).fill_(SENTINEL)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    w = buf.view(torch.int32).cpu().numpy()
    return bool((w[:GUARD] == SENTINEL).all() and (w[GUARD + n:] == SENTINEL).all())


def _raw_l1_ssim(img, gt, w_l1, w_ssim, dev):
    """r2_loss_l1_ssim on guarded sub-ranges: -> (grad, scratch, scalars) host arrays, after asserting every guard word."""
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd._C import _stream
    L = _lib.lib()
    H, W = img.shape
    x, y = torch.from_numpy(img).to(dev), torch.from_numpy(gt).to(dev)
    ns = int(L.r2_loss_l1_ssim_scratch_floats(W, H))
    bg, g = _guarded(H * W, dev)
    bs, s = _guarded(ns, dev)
    bc, c = _guarded(3, dev)
    rc = L.r2_loss_l1_ssim(W, H, x.data_ptr(), y.data_ptr(), w_l1, w_ssim, g.data_ptr(), s.data_ptr(), c.data_ptr(),
                           _stream(dev))
    _lib.check(rc, "r2_loss_l1_ssim")
    torch.cuda.synchronize()
    for buf, n, what in ((bg, H * W, "dL_dimg"), (bs, ns, "scratch"), (bc, 3, "scalars")):
        assert _guards_intact(buf, n), "r2_loss_l1_ssim %dx%d wrote outside %s" % (H, W, what)
    gw = g.view(torch.int32).cpu().numpy()
    assert not (gw == SENTINEL).any(), "a gradient element was not written"
    return g.cpu().numpy().reshape(H, W), s.cpu().numpy(), c.cpu().numpy()


def _raw_tv3d(vol, dev):
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd._C import _stream
    L = _lib.lib()
    n = vol.size
    v = torch.from_numpy(vol).to(dev)
    ns = int(L.r2_loss_tv3d_scratch_floats(*vol.shape))
    bg, g = _guarded(n, dev)
    bs, s = _guarded(ns, dev)
    bc, c = _guarded(2, dev)
    rc = L.r2_loss_tv3d(*vol.shape, v.data_ptr(), 1.0, g.data_ptr(), s.data_ptr(), c.data_ptr(), _stream(dev))
    _lib.check(rc, "r2_loss_tv3d")
    torch.cuda.synchronize()
    for buf, m, what in ((bg, n, "dL_dvol"), (bs, ns, "scratch"), (bc, 2, "scalars")):
        assert _guards_intact(buf, m), "r2_loss_tv3d %s wrote outside %s" % (vol.shape, what)
    assert not (g.view(torch.int32).cpu().numpy() == SENTINEL).any(), "a gradient element was not written"
    return g.cpu().numpy().reshape(vol.shape), s.cpu().numpy(), c.cpu().numpy()


ABI_IMAGES = [(1, 1), (1, 37), (37, 1), (5, 7), (15, 17), (17, 15), (33, 31), (16, 4096), (4096, 16)]


@pytest.mark.parametrize("hw", ABI_IMAGES, ids=["%dx%d" % s for s in ABI_IMAGES])
def test_l1_ssim_abi_writes_stay_inside_their_buffers(hw, gpu):
    img, gt = _images(hw, "ties")
    g, _s, c = _raw_l1_ssim(img, gt, 1.0, 0.25, gpu)
    r = R.l1_ssim64(img, gt, 1.0, 0.25)
    b = R.l1_ssim_bounds(r)
    assert (np.abs(g - r["grad"]) <= b["grad"]).all()
    assert abs(c[2] - r["loss"]) <= b["loss"]


ABI_VOLUMES = [(1, 1, 1), (1, 1, 4), (2, 1, 1), (1, 17, 33), (33, 1, 65), (5, 7, 6), (3, 300, 1)]


@pytest.mark.parametrize("shape", ABI_VOLUMES, ids=["x".join(map(str, s)) for s in ABI_VOLUMES])
def test_tv3d_abi_writes_stay_inside_their_buffers(shape, gpu):
    vol = _volume(shape, "integer")
    g, _s, c = _raw_tv3d(vol, gpu)
    ref, grad, _total, cnt = R.tv3d64(vol)
    assert np.array_equal(g == 0, grad == 0)
    if cnt == 0:
        assert math.isnan(c[0]) and math.isnan(c[1])
    else:
        assert abs(c[0] - ref) <= R.tv3d_bounds(vol, _total, cnt, grad)["tv"]


def test_l1_ssim_fold_at_2048(gpu):
    """The scalars of 2048^2 (16 384 per-block sums) against float64, and what the former float fold of the same per-block
    sums would have given (emulated bit for bit from the partials the kernel left in its scratch), both logged."""
    img, gt = _images((2048, 2048), "rand", seed=1)
    g, s, c = _raw_l1_ssim(img, gt, 1.0, 0.25, gpu)
    r = R.l1_ssim64(img, gt, 1.0, 0.25)
    b = R.l1_ssim_bounds(r)
    N = img.size
    off = (3 * N + 1) & ~1
    parts = s[off:off + 2 * R.n_blocks(*img.shape)].reshape(-1, 2)
    ssim32 = float(np.float32(R.float_fold(parts[:, 0]) / np.float32(N)))
    l132 = float(np.float32(R.float_fold(parts[:, 1]) / np.float32(N)))
    Hh.PARITY_LOG.append(dict(kind="loss_fold", case="l1_ssim_2048", ssim_err=abs(float(c[1]) - r["ssim"]),
                              ssim_err_float_fold=abs(ssim32 - r["ssim"]), ssim_bound=b["ssim"],
                              ssim_float_fold_bound=b["ssim_float_fold"], l1_err=abs(float(c[0]) - r["l1"]),
                              l1_err_float_fold=abs(l132 - r["l1"]), l1_bound=b["l1"]))
    assert abs(c[1] - r["ssim"]) <= b["ssim"] and abs(c[0] - r["l1"]) <= b["l1"]
    # the double fold of the partials is exact to ~nb * 2^-53: the scalar is the float-rounded float64 sum of the partials
    assert c[1] == np.float32(parts[:, 0].astype(np.float64).sum() / N)
    assert c[0] == np.float32(parts[:, 1].astype(np.float64).sum() / N)


def test_tv3d_fold_at_256(gpu):
    vol = _volume((256, 256, 256), "rand")
    _g, s, c = _raw_tv3d(vol, gpu)
    ref, grad, total, cnt = R.tv3d64(vol)
    b = R.tv3d_bounds(vol, total, cnt, grad)
    tv32 = float(np.float32(R.float_fold(s) * np.float32(1.0 / cnt)))
    Hh.PARITY_LOG.append(dict(kind="loss_fold", case="tv3d_256", tv_err=abs(float(c[0]) - ref),
                              tv_err_float_fold=abs(tv32 - ref), tv_bound=b["tv"], tv_float_fold_bound=b["tv_float_fold"]))
    assert abs(c[0] - ref) <= b["tv"]
    assert c[0] == np.float32(s.astype(np.float64).sum() / cnt)


# ----------------------------------------------------------------------------------------------------- determinism
def test_losses_are_bit_reproducible(gpu):
    from r2_gaussian_amd.losses import image_loss, tv_3d_loss
    img, gt = _images((1024, 1024), "rand", seed=2)
    vol = _volume((256, 256, 256), "rand")
    runs = []
    for _ in range(2):
        a = torch.from_numpy(img).to(gpu).requires_grad_(True)
        loss, parts = image_loss(a, torch.from_numpy(gt).to(gpu), 0.25)
        loss.backward()
        v = torch.from_numpy(vol).to(gpu).requires_grad_(True)
        tv = tv_3d_loss(v)
        tv.backward()
        torch.cuda.synchronize()
        runs.append([t.detach().cpu().view(torch.int32) for t in (parts, a.grad, tv.reshape(1), v.grad)])
    for x, y in zip(*runs):
        assert torch.equal(x, y)


# -------------------------------------------------------------------------------------------- wrapper semantics
def _loss_and_grad(image, gt, lam=0.25):
    from r2_gaussian_amd.losses import image_loss
    a = image.detach().clone().requires_grad_(True) if image.is_leaf else image
    loss, parts = image_loss(a, gt, lam)
    loss.backward()
    torch.cuda.synchronize()
    return parts.cpu(), (a.grad if a.is_leaf else None)


def test_image_loss_wrapper_layouts_and_dtypes(gpu):
    img, gt = _images((37, 53), "ties")
    x, y = torch.from_numpy(img).to(gpu), torch.from_numpy(gt).to(gpu)
    p0, g0 = _loss_and_grad(x[None], y[None])
    bits = lambda t: t.detach().float().cpu().view(torch.int32)
    # [H, W] and [1, H, W], either way round
    p1, g1 = _loss_and_grad(x, y)
    assert torch.equal(p1.view(torch.int32), p0.view(torch.int32)) and g1.shape == (37, 53)
    assert torch.equal(bits(g1), bits(g0[0]))
    p1, _ = _loss_and_grad(x, y[None])
    assert torch.equal(p1.view(torch.int32), p0.view(torch.int32))
    # a transposed view and a strided slice of a batch
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous()
    p1, g1 = _loss_and_grad(xt, y)
    assert torch.equal(p1.view(torch.int32), p0.view(torch.int32)) and torch.equal(bits(g1), bits(g0[0]))
    batch = torch.zeros(37, 3, 53, device=gpu)
    batch[:, 1] = x
    leaf = batch.requires_grad_(True)
    p1, _ = _loss_and_grad(leaf[:, 1], y)
    assert torch.equal(p1.view(torch.int32), p0.view(torch.int32))
    assert torch.equal(bits(leaf.grad[:, 1]), bits(g0[0])) and not leaf.grad[:, 0].any() and not leaf.grad[:, 2].any()
    # gt on the host or in another dtype
    p1, _ = _loss_and_grad(x, y.cpu())
    assert torch.equal(p1.view(torch.int32), p0.view(torch.int32))
    p1, _ = _loss_and_grad(x, y.double())
    assert torch.equal(p1.view(torch.int32), p0.view(torch.int32))
    # float64 / bfloat16 images: computed on the float32 values, the gradient comes back in the input's dtype
    p1, g1 = _loss_and_grad(x.double(), y)
    assert g1.dtype == torch.float64 and torch.equal(p1.view(torch.int32), p0.view(torch.int32))
    assert torch.equal(bits(g1), bits(g0[0]))
    xb = x.bfloat16()
    pb, gb = _loss_and_grad(xb, y)
    pr, gr = _loss_and_grad(xb.float(), y)
    assert gb.dtype == torch.bfloat16 and torch.equal(pb.view(torch.int32), pr.view(torch.int32))
    assert torch.equal(gb.cpu(), gr.bfloat16().cpu())


def test_image_loss_used_twice_in_one_graph(gpu):
    from r2_gaussian_amd.losses import image_loss
    img, gt = _images((40, 48), "rand")
    _, gt2 = _images((40, 48), "rand", seed=5)
    x = torch.from_numpy(img).to(gpu)
    y, y2 = torch.from_numpy(gt).to(gpu), torch.from_numpy(gt2).to(gpu)
    a = x.clone().requires_grad_(True)
    l1, _ = image_loss(a, y, 0.25)
    l2, _ = image_loss(a, y2, 1.0)
    (l1 + 0.5 * l2).backward()
    _, g1 = _loss_and_grad(x, y, 0.25)
    _, g2 = _loss_and_grad(x, y2, 1.0)
    torch.cuda.synchronize()
    want = g1.double() + 0.5 * g2.double()
    assert (torch.abs(a.grad.double() - want) <= R.U * torch.abs(want) * 2).all()


def test_image_loss_rejects_a_larger_gt(gpu):
    """gt larger than the image (the kernel would read it with the image's W and H): a ValueError before any launch."""
    from r2_gaussian_amd.losses import image_loss
    x = torch.rand(1, 20, 30, device=gpu)
    for gt in (torch.rand(1, 20, 31, device=gpu), torch.rand(1, 21, 30, device=gpu), torch.rand(30, 30, device=gpu)):
        with pytest.raises(ValueError):
            image_loss(x, gt)
    with pytest.raises(ValueError):
        image_loss(torch.rand(2, 20, 30, device=gpu), torch.rand(2, 20, 30, device=gpu))


def test_tv3d_wrapper_strided_and_dtypes(gpu):
    from r2_gaussian_amd.losses import tv_3d_loss
    vol = torch.from_numpy(_volume((9, 12, 7), "rand")).to(gpu)
    a = vol.clone().requires_grad_(True)
    t0 = tv_3d_loss(a)
    t0.backward()
    base = vol.permute(2, 0, 1).contiguous().requires_grad_(True)      # [7, 9, 12] storage, viewed back as [9, 12, 7]
    view = base.permute(1, 2, 0)
    assert not view.is_contiguous()
    t1 = tv_3d_loss(view)
    t1.backward()
    torch.cuda.synchronize()
    assert torch.equal(t1.view(1).view(torch.int32), t0.view(1).view(torch.int32))
    assert torch.equal(base.grad.permute(1, 2, 0).contiguous().view(torch.int32), a.grad.view(torch.int32))
    d = vol.double().requires_grad_(True)
    tv_3d_loss(d).backward()
    assert d.grad.dtype == torch.float64 and torch.equal(d.grad.float(), a.grad)


# ---------------------------------------------------------------------------------------- against the metrics kernel
@pytest.mark.parametrize("hw", [(33, 31), (256, 256), (1024, 1024)], ids=["33x31", "256", "1024"])
def test_loss_ssim_equals_slice_metrics(hw, gpu):
    """The loss's SSIM part and metrics.slice_metrics of the same image as a 1 x H x W array (axis 0): both blur with
    ssim_window.hpp and fold in double, so each is within the derived bound of float64 and they agree to the sum of both."""
    from r2_gaussian_amd import metrics as M
    from r2_gaussian_amd.losses import image_loss
    img, gt = _images(hw, "blob" if hw[0] == 256 else "rand")
    x, y = torch.from_numpy(img).to(gpu), torch.from_numpy(gt).to(gpu)
    _, parts = image_loss(x, y, 0.25)
    tab = M.slice_metrics(y[None], x[None], 0)
    torch.cuda.synchronize()
    r = R.l1_ssim64(img, gt, 1.0, 0.25)
    b = R.l1_ssim_bounds(r)
    s_loss, s_metric = float(parts[1]), float(tab[0, 0])
    Hh.PARITY_LOG.append(dict(kind="loss_vs_metric", case="%dx%d" % hw, diff=abs(s_loss - s_metric),
                              loss_err=abs(s_loss - r["ssim"]), metric_err=abs(s_metric - r["ssim"]), bound=b["ssim"]))
    assert abs(s_loss - r["ssim"]) <= b["ssim"] and abs(s_metric - r["ssim"]) <= b["ssim"]
    assert abs(s_loss - s_metric) <= 2 * b["ssim"]
