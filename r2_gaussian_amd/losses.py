"""The training loop's loss stack on the MI355X kernels (csrc/loss_ops.hip): drop-in replacements for
``l1_loss + lambda_dssim * (1 - ssim)`` and ``tv_3d_loss(vol, "mean")`` of r2_gaussian/utils/loss_utils.py, each as ONE
autograd node whose forward already computes the gradient (two / one kernel launches instead of ~60 torch kernels, and no
vendor convolution).  The results are device scalars: nothing here synchronises with the host (train.py:204-209 calls
``.item()`` on every loss every iteration; read the tensors only when something is logged).
"""
import torch

from . import _lib
from ._boundary import _F32, call, ptr_table, require_gpu


def _check_image_shapes(image, gt):
    """One [H, W] or [1, H, W] projection and a ground truth of the same size (the kernel reads gt with the image's W and H:
    a mismatch would be a silently wrong value or a read past gt's end).  The reference raises a shape error here too."""
    for name, t in (("image", image), ("gt", gt)):
        if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != 1):
            raise ValueError("%s must be [H, W] or [1, H, W], got %s" % (name, tuple(t.shape)))
    if tuple(gt.shape[-2:]) != tuple(image.shape[-2:]):
        raise ValueError("gt is %s but the image is %s" % (tuple(gt.shape[-2:]), tuple(image.shape[-2:])))


class _ImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, w_l1, w_ssim):
        _check_image_shapes(image, gt)
        require_gpu(image, "image")
        img = image.reshape(image.shape[-2], image.shape[-1]).to(_F32).contiguous()
        ref = gt.reshape(gt.shape[-2], gt.shape[-1]).to(device=img.device, dtype=_F32).contiguous()
        H, W = img.shape
        grad = torch.empty_like(img)
        scratch = torch.empty(_lib.lib().r2_loss_l1_ssim_scratch_floats(W, H), dtype=_F32, device=img.device)
        scalars = torch.empty(3, dtype=_F32, device=img.device)
        call("r2_loss_l1_ssim", img.device, W, H, img, ref, float(w_l1), float(w_ssim), grad, scratch, scalars)
        ctx.save_for_backward(grad)
        ctx.shape, ctx.dtype = image.shape, image.dtype
        ctx.mark_non_differentiable(scalars)
        return scalars[2], scalars

    @staticmethod
    def backward(ctx, g, _):
        (grad,) = ctx.saved_tensors
        return (grad * g).reshape(ctx.shape).to(ctx.dtype), None, None, None


def _check_weight_shape(name, w, hw):
    """One view's weights: a [H, W] or [1, H, W] tensor of the image's size (the kernel reads it with the image's W and H)."""
    if not torch.is_tensor(w) or w.dim() not in (2, 3) or (w.dim() == 3 and w.shape[0] != 1):
        raise ValueError("%s must be [H, W] or [1, H, W], got %s" % (name, tuple(w.shape) if torch.is_tensor(w) else
                                                                     type(w).__name__))
    if w.is_complex():
        raise ValueError("%s must be real or bool, got %s" % (name, w.dtype))
    if tuple(w.shape[-2:]) != tuple(hw):
        raise ValueError("%s is %s but the image is %s" % (name, tuple(w.shape[-2:]), tuple(hw)))


def _weights_f32(w, H, W, dev):
    """Weights as the kernels read them, converted the way gt is: float32, contiguous, on the image's device (bool -> 0 / 1)."""
    return w.detach().reshape(H, W).to(device=dev, dtype=_F32).contiguous()


class _WeightedImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, weights, w_l1, w_ssim):
        _check_image_shapes(image, gt)
        _check_weight_shape("weights", weights, image.shape[-2:])
        require_gpu(image, "image")
        img = image.reshape(image.shape[-2], image.shape[-1]).to(_F32).contiguous()
        ref = gt.reshape(gt.shape[-2], gt.shape[-1]).to(device=img.device, dtype=_F32).contiguous()
        H, W = img.shape
        wts = _weights_f32(weights, H, W, img.device)
        grad = torch.empty_like(img)
        scratch = torch.empty(_lib.lib().r2_loss_l1_ssim_weighted_scratch_floats(W, H), dtype=_F32, device=img.device)
        scalars = torch.empty(4, dtype=_F32, device=img.device)
        call("r2_loss_l1_ssim_weighted", img.device, W, H, img, ref, wts, float(w_l1), float(w_ssim), grad, scratch, scalars)
        ctx.save_for_backward(grad)
        ctx.shape, ctx.dtype = image.shape, image.dtype
        ctx.mark_non_differentiable(scalars)
        return scalars[2], scalars

    @staticmethod
    def backward(ctx, g, _):
        (grad,) = ctx.saved_tensors
        return (grad * g).reshape(ctx.shape).to(ctx.dtype), None, None, None, None


def image_loss(image, gt, lambda_dssim=0.25, weights=None):
    """-> (loss, parts): loss = L1 + lambda_dssim * (1 - SSIM) as a device scalar with a gradient; parts = tensor
    {l1, ssim, loss} for logging (train.py:118-126).
    weights ([H, W] or [1, H, W]; any real or bool dtype, device and strides; never differentiated): the weighted loss of
    r2_loss_l1_ssim_weighted (include/r2hip.h) -- sums weighted per pixel and normalised by the weights' sum, a weight that is
    not > 0 (also NaN) marks an unmeasured pixel whose gt is never used (it may be NaN), no measured pixel at all gives a
    loss of 0 with a zero gradient -- and parts = {l1, ssim, loss, sum of the weights}.  None: the unweighted call, untouched."""
    if weights is None:
        return _ImageLoss.apply(image, gt, 1.0, float(lambda_dssim))
    _check_image_shapes(image, gt)
    _check_weight_shape("weights", weights, image.shape[-2:])
    return _WeightedImageLoss.apply(image, gt, weights, 1.0, float(lambda_dssim))


def _check_batch_shapes(images, gts):
    """[V, H, W] projections and V ground truths: a sequence of [H, W] / [1, H, W] tensors or one [V, H, W] tensor."""
    if not torch.is_tensor(images) or images.dim() != 3 or images.shape[0] < 1:
        raise ValueError("images must be [V, H, W] with V >= 1, got %s" % (tuple(images.shape) if torch.is_tensor(images) else
                                                                           type(images).__name__,))
    V, hw = images.shape[0], tuple(images.shape[1:])
    if torch.is_tensor(gts):
        if gts.dim() != 3 or tuple(gts.shape) != (V,) + hw:
            raise ValueError("gts is %s but the images are %s" % (tuple(gts.shape), tuple(images.shape)))
        return
    gts = list(gts)
    if len(gts) != V:
        raise ValueError("%d ground truths for %d images" % (len(gts), V))
    for k, t in enumerate(gts):
        if not torch.is_tensor(t) or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != 1):
            raise ValueError("gts[%d] must be [H, W] or [1, H, W], got %s" % (k, tuple(t.shape) if torch.is_tensor(t) else
                                                                              type(t).__name__))
        if tuple(t.shape[-2:]) != hw:
            raise ValueError("gts[%d] is %s but the images are %s" % (k, tuple(t.shape[-2:]), hw))


class _ImageLossBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, gts, w_l1, w_ssim):
        _check_batch_shapes(images, gts)
        require_gpu(images, "images")
        img = images.to(_F32).contiguous()
        V, H, W = img.shape
        # the ground truths are read where they lie; only one on another device / of another type / strided is converted
        refs = list(gts.to(device=img.device, dtype=_F32).contiguous()) if torch.is_tensor(gts) else [
            t.reshape(H, W).to(device=img.device, dtype=_F32).contiguous() for t in gts]
        grad = torch.empty_like(img)
        scratch = torch.empty(_lib.lib().r2_loss_l1_ssim_batch_scratch_floats(V, W, H), dtype=_F32, device=img.device)
        scalars = torch.empty((V + 1, 3), dtype=_F32, device=img.device)
        call("r2_loss_l1_ssim_batch", img.device, V, W, H, img, ptr_table(refs), float(w_l1), float(w_ssim), grad, scratch,
             scalars)
        ctx.save_for_backward(grad)
        ctx.dtype = images.dtype
        ctx.mark_non_differentiable(scalars)
        return scalars[V, 2], scalars

    @staticmethod
    def backward(ctx, g, _):
        (grad,) = ctx.saved_tensors
        return (grad * g).to(ctx.dtype), None, None, None


def _check_batch_weights(images, weights):
    """V views' weights: one [V, H, W] tensor, or a sequence of V items, each None (unit weights) or one view's weights.
    -> the tensor, or the sequence as a list."""
    V, hw = images.shape[0], tuple(images.shape[1:])
    if torch.is_tensor(weights):
        if weights.dim() != 3 or tuple(weights.shape) != (V,) + hw:
            raise ValueError("weights is %s but the images are %s" % (tuple(weights.shape), tuple(images.shape)))
        if weights.is_complex():
            raise ValueError("weights must be real or bool, got %s" % (weights.dtype,))
        return weights
    weights = list(weights)
    if len(weights) != V:
        raise ValueError("%d weights for %d images" % (len(weights), V))
    for k, w in enumerate(weights):
        if w is not None:
            _check_weight_shape("weights[%d]" % k, w, hw)
    return weights


class _WeightedImageLossBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, gts, weights, w_l1, w_ssim):
        _check_batch_shapes(images, gts)
        weights = _check_batch_weights(images, weights)
        require_gpu(images, "images")
        img = images.to(_F32).contiguous()
        V, H, W = img.shape
        refs = list(gts.to(device=img.device, dtype=_F32).contiguous()) if torch.is_tensor(gts) else [
            t.reshape(H, W).to(device=img.device, dtype=_F32).contiguous() for t in gts]
        # like the ground truths, weights given one by one are read where they lie
        wts = list(weights.detach().to(device=img.device, dtype=_F32).contiguous()) if torch.is_tensor(weights) else [
            None if w is None else _weights_f32(w, H, W, img.device) for w in weights]
        grad = torch.empty_like(img)
        scratch = torch.empty(_lib.lib().r2_loss_l1_ssim_weighted_batch_scratch_floats(V, W, H), dtype=_F32, device=img.device)
        scalars = torch.empty((V + 1, 4), dtype=_F32, device=img.device)
        call("r2_loss_l1_ssim_weighted_batch", img.device, V, W, H, img, ptr_table(refs), ptr_table(wts), float(w_l1),
             float(w_ssim), grad, scratch, scalars)
        ctx.save_for_backward(grad)
        ctx.dtype = images.dtype
        ctx.mark_non_differentiable(scalars)
        return scalars[V, 2], scalars

    @staticmethod
    def backward(ctx, g, _):
        (grad,) = ctx.saved_tensors
        return (grad * g).to(ctx.dtype), None, None, None, None


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
    _check_batch_shapes(images, gts)
    if weights is None:
        return _ImageLossBatch.apply(images, gts if torch.is_tensor(gts) else list(gts), 1.0, float(lambda_dssim))
    weights = _check_batch_weights(images, weights)
    return _WeightedImageLossBatch.apply(images, gts if torch.is_tensor(gts) else list(gts), weights, 1.0, float(lambda_dssim))


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
