"""GPU: the batched image loss (r2_loss_l1_ssim_batch, losses.image_loss_batch) -- bit for bit against the single-view kernels
it shares its device code with, against the float64 restatement of tests/loss_ref.py within the tolerance
tests/test_losses_gpu.py applies to image_loss, its autograd node, and its determinism."""
import numpy as np
import pytest
import torch

from tests import loss_ref as R

pytestmark = pytest.mark.gpu

SIZES = {"37x53": (37, 53), "128": (128, 128), "512": (512, 512)}
CASES = [(V, s, lam) for s in ("37x53", "128") for V in (1, 2, 5, 8) for lam in (0.0, 0.25)] + [(8, "512", 0.25)]
IDS = ["V%d_%s_lam%g" % c for c in CASES]


def _inputs(V, hw, gpu, seed=0):
    """Random images [V, H, W] with exact zeros of img - gt, and V separately allocated ground truths."""
    g = torch.Generator().manual_seed(1000 * V + hw[0] + seed)
    gts = [torch.rand(*hw, generator=g) for _ in range(V)]
    img = torch.stack([(t + 0.1 * torch.randn(*hw, generator=g)).clamp_min(0.0) for t in gts])
    img[:, :4, :4] = torch.stack(gts)[:, :4, :4]
    return img.to(gpu), [t.to(gpu) for t in gts]


def _single(img, gt, w_l1, w_ssim):
    """r2_loss_l1_ssim on one view with explicit float weights -> (grad [H, W], scalars [3])."""
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    H, W = img.shape
    img, gt = img.contiguous(), gt.contiguous()
    grad = torch.empty_like(img)
    scratch = torch.empty(L.r2_loss_l1_ssim_scratch_floats(W, H), dtype=torch.float32, device=img.device)
    scalars = torch.empty(3, dtype=torch.float32, device=img.device)
    rc = L.r2_loss_l1_ssim(W, H, img.data_ptr(), gt.data_ptr(), float(w_l1), float(w_ssim), grad.data_ptr(), scratch.data_ptr(),
                           scalars.data_ptr(), None)
    _lib.check(rc, "r2_loss_l1_ssim")
    torch.cuda.synchronize()
    return grad, scalars


def _batch(img, gts, lam):
    from r2_gaussian_amd.losses import image_loss_batch
    x = img.clone().requires_grad_(True)
    loss, parts = image_loss_batch(x, gts, lam)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), parts, x.grad


def _mean_row(parts, V):
    """The float64 mean of the V float rows, in view order, cast to float."""
    rows = parts[:V].cpu().numpy().astype(np.float64)
    acc = np.zeros(3)
    for v in range(V):
        acc = acc + rows[v]
    return (acc / V).astype(np.float32)


def _check_against_single(img, gts, lam, loss, parts, grad):
    V = img.shape[0]
    w1, ws = np.float32(1.0) / np.float32(V), np.float32(lam) / np.float32(V)   # the quotients formed in float
    assert parts.shape == (V + 1, 3) and grad.shape == img.shape
    for v in range(V):
        _g, scal = _single(img[v], gts[v], 1.0, lam)
        assert torch.equal(parts[v], scal), (v, parts[v], scal)
        gv, _s = _single(img[v], gts[v], w1, ws)
        assert torch.equal(grad[v], gv), (v, float((grad[v] - gv).abs().max()))
    assert np.array_equal(parts[V].cpu().numpy(), _mean_row(parts, V))
    assert torch.equal(loss, parts[V, 2])


@pytest.mark.parametrize("V,size,lam", CASES, ids=IDS)
def test_bit_identical_to_the_single_view_kernels(V, size, lam, gpu):
    img, gts = _inputs(V, SIZES[size], gpu)
    _check_against_single(img, gts, lam, *_batch(img, gts, lam))


@pytest.mark.parametrize("V,size,lam", CASES, ids=IDS)
def test_against_float64(V, size, lam, gpu):
    """Per view, the tolerance of tests/test_losses_gpu.py:26-31: value 2e-6 relative + 1e-7, l1 1e-6, ssim 2e-6, gradient
    2e-5 of its largest magnitude -- the gradient's scale taken after the division by V."""
    img, gts = _inputs(V, SIZES[size], gpu)
    loss, parts, grad = _batch(img, gts, lam)
    parts, grad = parts.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)
    refs = [R.l1_ssim64(img[v].cpu().numpy(), gts[v].cpu().numpy(), 1.0, lam) for v in range(V)]
    worst = dict(loss=0.0, l1=0.0, ssim=0.0, grad=0.0)
    for v, r in enumerate(refs):
        worst["loss"] = max(worst["loss"], abs(parts[v, 2] - r["loss"]) / (2e-6 * abs(r["loss"]) + 1e-7))
        worst["l1"] = max(worst["l1"], abs(parts[v, 0] - r["l1"]) / 1e-6)
        worst["ssim"] = max(worst["ssim"], abs(parts[v, 1] - r["ssim"]) / 2e-6)
        want = r["grad"] / V
        worst["grad"] = max(worst["grad"], np.abs(grad[v] - want).max() / (2e-5 * np.abs(want).max()))
    mean = {k: float(np.mean([r[k] for r in refs])) for k in ("loss", "l1", "ssim")}
    batch = dict(loss=abs(parts[V, 2] - mean["loss"]) / (2e-6 * abs(mean["loss"]) + 1e-7), l1=abs(parts[V, 0] - mean["l1"]) / 1e-6,
                 ssim=abs(parts[V, 1] - mean["ssim"]) / 2e-6)
    print("fractions of the tolerance: per view %s, batch row %s" % (worst, batch))
    assert float(loss) == parts[V, 2]
    assert all(x <= 1.0 for x in worst.values()), worst
    assert all(x <= 1.0 for x in batch.values()), batch


def test_upstream_gradient_scales(gpu):
    from r2_gaussian_amd.losses import image_loss_batch
    img, gts = _inputs(3, (50, 70), gpu)
    _l, _p, g1 = _batch(img, gts, 0.25)
    x = img.clone().requires_grad_(True)
    (3 * image_loss_batch(x, gts, 0.25)[0]).backward()
    torch.cuda.synchronize()
    assert torch.equal(x.grad, 3 * g1)


def test_one_view_is_image_loss(gpu):
    from r2_gaussian_amd.losses import image_loss
    img, gts = _inputs(1, (50, 70), gpu)
    loss, parts, grad = _batch(img, gts, 0.25)
    x = img[0].clone().requires_grad_(True)
    l1, p1 = image_loss(x, gts[0], 0.25)
    l1.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss, l1.detach()) and torch.equal(parts[0], p1) and torch.equal(parts[1], p1)
    assert torch.equal(grad[0], x.grad)


def test_stacked_and_listed_ground_truths_agree(gpu):
    img, gts = _inputs(4, (37, 53), gpu)
    a = _batch(img, torch.stack(gts), 0.25)
    b = _batch(img, [t[None] for t in gts], 0.25)
    c = _batch(img, gts, 0.25)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_shape_errors(gpu):
    from r2_gaussian_amd.losses import image_loss_batch
    img, gts = _inputs(3, (37, 53), gpu)
    with pytest.raises(ValueError):
        image_loss_batch(img, [])
    with pytest.raises(ValueError):
        image_loss_batch(img, gts[:2])
    with pytest.raises(ValueError):
        image_loss_batch(img, gts[:2] + [gts[2][:, :52]])
    with pytest.raises(ValueError):
        image_loss_batch(img, torch.stack(gts)[:, :36])
    with pytest.raises(ValueError):
        image_loss_batch(img[0], gts[:1])


def test_more_views_than_one_pointer_chunk(gpu):
    """R2_LOSS_BATCH_CHUNK + 1 views: two pairs of launches, the last one with a single view, which also writes the batch row."""
    from r2_gaussian_amd import _lib
    V = _lib.R2_LOSS_BATCH_CHUNK + 1
    img, gts = _inputs(V, (37, 53), gpu)
    _check_against_single(img, gts, 0.25, *_batch(img, gts, 0.25))


def test_library_rejects_invalid_arguments(gpu):
    import ctypes as C
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    img, gts = _inputs(2, (37, 53), gpu)
    out, scal = torch.empty_like(img), torch.empty((3, 3), device=gpu)
    scratch = torch.empty(L.r2_loss_l1_ssim_batch_scratch_floats(2, 53, 37), device=gpu)
    good = (C.c_void_p * 2)(gts[0].data_ptr(), gts[1].data_ptr())
    hole = (C.c_void_p * 2)(gts[0].data_ptr(), None)

    def call(V=2, W=53, H=37, x=img.data_ptr(), table=good, g=out.data_ptr(), s=scratch.data_ptr(), c=scal.data_ptr()):
        return L.r2_loss_l1_ssim_batch(V, W, H, x, table, 1.0, 0.25, g, s, c, None)
    assert call() == 0
    for kw in (dict(V=0), dict(W=0), dict(H=-1), dict(x=None), dict(table=None), dict(table=hole), dict(g=None), dict(s=None),
               dict(c=None)):
        assert call(**kw) == _lib.R2_ERR_INVALID, kw
        assert b"r2_loss_l1_ssim_batch" in L.r2_last_error()
    assert L.r2_loss_l1_ssim_batch_scratch_floats(0, 53, 37) == 0
    torch.cuda.synchronize()


def test_two_calls_are_bit_identical(gpu):
    img, gts = _inputs(5, (128, 128), gpu)
    a, b = _batch(img, gts, 0.25), _batch(img, gts, 0.25)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
