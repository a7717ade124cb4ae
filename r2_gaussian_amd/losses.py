"""The training loop's loss stack on the MI355X kernels (csrc/loss_ops.hip): drop-in replacements for
``l1_loss + lambda_dssim * (1 - ssim)`` and ``tv_3d_loss(vol, "mean")`` of r2_gaussian/utils/loss_utils.py, each as ONE
autograd node whose forward already computes the gradient (two / one kernel launches instead of ~60 torch kernels, and no
vendor convolution).  The results are device scalars: nothing here synchronises with the host (train.py:204-209 calls
``.item()`` on every loss every iteration; read the tensors only when something is logged).
"""
import torch

from . import _lib
from ._boundary import _F32, call, ptr_table, require_gpu


def _check_view(name, t, hw=None, whose="the image is", real=False):
    """One view's image, ground truth or weights: a [H, W] or [1, H, W] tensor, of the size hw where one is given (the
    kernels read every array with the image's W and H: a mismatch would be a silently wrong value or a read past its end;
    the reference raises a shape error here too).  real: weights are of a real or bool dtype."""
    if not torch.is_tensor(t) or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != 1):
        raise ValueError("%s must be [H, W] or [1, H, W], got %s" % (name, tuple(t.shape) if torch.is_tensor(t) else
                                                                     type(t).__name__))
    if real and t.is_complex():
        raise ValueError("%s must be real or bool, got %s" % (name, t.dtype))
    if hw is not None and tuple(t.shape[-2:]) != tuple(hw):
        raise ValueError("%s is %s but %s %s" % (name, tuple(t.shape[-2:]), whose, tuple(hw)))


def _check_image_shapes(image, gt, weights=None):
    """One projection, its ground truth and, where given, its weights."""
    _check_view("image", image)
    _check_view("gt", gt, image.shape[-2:])
    if weights is not None:
        _check_view("weights", weights, image.shape[-2:], real=True)


def _check_batch_shapes(images, gts, weights=None):
    """[V, H, W] projections and V ground truths: a sequence of [H, W] / [1, H, W] tensors or one [V, H, W] tensor.  weights:
    None, one [V, H, W] tensor, or a sequence of V items, each None (unit weights) or one view's weights.
    -> (gts, weights), the sequences as lists."""
    if not torch.is_tensor(images) or images.dim() != 3 or images.shape[0] < 1:
        raise ValueError("images must be [V, H, W] with V >= 1, got %s" % (tuple(images.shape) if torch.is_tensor(images) else
                                                                           type(images).__name__,))
    V, hw = images.shape[0], tuple(images.shape[1:])
    if torch.is_tensor(gts):
        if gts.dim() != 3 or tuple(gts.shape) != (V,) + hw:
            raise ValueError("gts is %s but the images are %s" % (tuple(gts.shape), tuple(images.shape)))
    else:
        gts = list(gts)
        if len(gts) != V:
            raise ValueError("%d ground truths for %d images" % (len(gts), V))
        for k, t in enumerate(gts):
            _check_view("gts[%d]" % k, t, hw, "the images are")
    if torch.is_tensor(weights):
        if weights.dim() != 3 or tuple(weights.shape) != (V,) + hw:
            raise ValueError("weights is %s but the images are %s" % (tuple(weights.shape), tuple(images.shape)))
        if weights.is_complex():
            raise ValueError("weights must be real or bool, got %s" % (weights.dtype,))
    elif weights is not None:
        weights = list(weights)
        if len(weights) != V:
            raise ValueError("%d weights for %d images" % (len(weights), V))
        for k, w in enumerate(weights):
            if w is not None:
                _check_view("weights[%d]" % k, w, hw, real=True)
    return gts, weights


def _views_f32(views, H, W, dev):
    """V views' ground truths or weights as the kernels read them: float32, contiguous, on the images' device (bool -> 0 / 1),
    never differentiated.  One [V, H, W] tensor gives its V rows; views given one by one are read where they lie (only one on
    another device / of another type / strided is converted), and a None among them stays (that view's unit weights)."""
    if torch.is_tensor(views):
        return list(views.detach().to(device=dev, dtype=_F32).contiguous())
    return [None if t is None else t.detach().reshape(H, W).to(device=dev, dtype=_F32).contiguous() for t in views]


class _ImageLoss(torch.autograd.Function):
    """The four entries r2_loss_l1_ssim[_weighted][_batch] on arguments whose shapes are checked: one view (batch False:
    image, gt and weights as image_loss takes them) or V (as image_loss_batch does); weights None: the unweighted entry."""

    @staticmethod
    def forward(ctx, images, gts, weights, batch, w_l1, w_ssim):
        require_gpu(images, "images" if batch else "image")
        H, W = images.shape[-2:]
        img = images.reshape(-1, H, W).to(_F32).contiguous()
        V, dev = img.shape[0], img.device
        views = [_views_f32(t if batch else [t], H, W, dev) for t in (gts, weights) if t is not None]
        entry = "r2_loss_l1_ssim" + ("_weighted" if weights is not None else "") + ("_batch" if batch else "")
        cols = 3 if weights is None else 4
        size = (V, W, H) if batch else (W, H)
        grad = torch.empty_like(img)
        scratch = torch.empty(getattr(_lib.lib(), entry + "_scratch_floats")(*size), dtype=_F32, device=dev)
        scalars = torch.empty((V + 1, cols) if batch else cols, dtype=_F32, device=dev)
        call(entry, dev, *size, img, *[ptr_table(t) if batch else t[0] for t in views], float(w_l1), float(w_ssim), grad,
             scratch, scalars)
        ctx.save_for_backward(grad)
        ctx.shape, ctx.dtype = images.shape, images.dtype
        ctx.mark_non_differentiable(scalars)
        return scalars[V, 2] if batch else scalars[2], scalars

    @staticmethod
    def backward(ctx, g, _):
        (grad,) = ctx.saved_tensors
        return (grad * g).reshape(ctx.shape).to(ctx.dtype), None, None, None, None, None


def image_loss(image, gt, lambda_dssim=0.25, weights=None):
    """-> (loss, parts): loss = L1 + lambda_dssim * (1 - SSIM) as a device scalar with a gradient; parts = tensor
    {l1, ssim, loss} for logging (train.py:118-126).
    weights ([H, W] or [1, H, W]; any real or bool dtype, device and strides; never differentiated): the weighted loss of
    r2_loss_l1_ssim_weighted (include/r2hip.h) -- sums weighted per pixel and normalised by the weights' sum, a weight that is
    not > 0 (also NaN) marks an unmeasured pixel whose gt is never used (it may be NaN), no measured pixel at all gives a
    loss of 0 with a zero gradient -- and parts = {l1, ssim, loss, sum of the weights}.  None: the unweighted call, untouched."""
    _check_image_shapes(image, gt, weights)
    return _ImageLoss.apply(image, gt, weights, False, 1.0, float(lambda_dssim))


def image_loss_batch(images, gts, lambda_dssim=0.25, weights=None):
    """`image_loss` of V views in two launches per 16 views and ONE autograd node.  images [V, H, W]; gts: a sequence of V
    tensors [H, W] / [1, H, W] (read in place: they need not be contiguous with each other) or one [V, H, W] tensor.
    -> (loss, parts): loss = the mean over the views of L1 + lambda_dssim * (1 - SSIM), a device scalar with a gradient;
    parts [V + 1, 3]: row v = {l1, ssim, loss} of view v, bit-identical to image_loss's, row V their means.  Shape errors
    raise ValueError before the library is touched.
    weights (one [V, H, W] tensor, or a sequence of V items, each None = unit weights or a tensor as image_loss takes it, read
    in place; never differentiated): the mean over the views of each view's own weighted loss, three launches per 16 views;
    parts [V + 1, 4]: row v = {l1, ssim, loss, sum of the weights} of view v, bit-identical to image_loss's, row V the means
    of the first three columns and the sum of the fourth.  None: the unweighted call, untouched."""
    gts, weights = _check_batch_shapes(images, gts, weights)
    return _ImageLoss.apply(images, gts, weights, True, 1.0, float(lambda_dssim))


class _TV3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vol):
        require_gpu(vol, "vol")
        v = vol.to(_F32).contiguous()
        nx, ny, nz = v.shape
        grad = torch.empty_like(v)
        scratch = torch.empty(_lib.lib().r2_loss_tv3d_scratch_floats(nx, ny, nz), dtype=_F32, device=v.device)
        scalars = torch.empty(2, dtype=_F32, device=v.device)
        call("r2_loss_tv3d", v.device, nx, ny, nz, v, 1.0, grad, scratch, scalars)
        ctx.save_for_backward(grad)
        ctx.dtype = vol.dtype
        return scalars[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g).to(ctx.dtype)


def tv_3d_loss(vol):
    """tv_3d_loss(vol, reduction="mean") of loss_utils.py:19-34 as one autograd node.  A volume without neighbour pairs
    (1 x 1 x 1) gives NaN and a zero gradient, as the reference's 0 / 0 does."""
    return _TV3D.apply(vol)
