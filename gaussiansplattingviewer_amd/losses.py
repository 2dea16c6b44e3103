"""The photometric loss of a 3D Gaussian Splatting fit, fused: L1 + D-SSIM of a rendered image
against its target in two HIP kernels per direction (gsr_image_loss and
gsr_image_loss_backward, include/gsr.h, which states the semantics).

    color, radii = GaussianRasterizer(settings)(...)
    loss = photometric_loss(color, target)          # (1 - 0.2) * L1 + 0.2 * (1 - SSIM)
    loss.backward()

The images are [C, H, W]; the channels are independent; SSIM is the reference's: an 11 x 11
Gaussian window of sigma 1.5, zero padding of 5, C1 = 0.01^2, C2 = 0.03^2, the mean over all
elements.  Only `image` gets a gradient: `target` is a constant.  The values and the gradient
have the same bits on every call with the same inputs (no atomics), so a fit rendered with
`deterministic=True` stays reproducible through its loss.

A strip image (`tile_rows=`) is an image like any other: its loss is that of the strip taken
alone, zero padded at the strip's edges, NOT the frame's loss restricted to the strip.  A halo
exchange between ranks, which that would take, is out of scope.

There is no fallback: without libgsr.so or a HIP device the calls raise.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib

LAMBDA_DSSIM = 0.2  # 3D Gaussian Splatting's weight of the D-SSIM term


def _stream(dev: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _inputs(image: torch.Tensor, target: torch.Tensor, lam: float) -> _lib.GsrImageLossInputs:
    C, H, W = image.shape
    return _lib.GsrImageLossInputs(C, H, W, lam, image.data_ptr(), target.data_ptr())


def image_loss_native(image, target, lambda_dssim=LAMBDA_DSSIM, need_saved=False):
    """gsr_image_loss by ctypes on torch's current stream -> (values [3] = loss, l1, ssim; saved
    [3, C, H, W], or None without `need_saved`).  `image` and `target` are contiguous float32
    [C, H, W] on one HIP device (`photometric_loss` makes them so)."""
    lib = _lib.load_library()
    workspace, forward, _ = _lib.image_loss_fns(lib)
    C, H, W = image.shape
    with torch.cuda.device(image.device):
        nbytes = _lib.check(workspace(C, H, W), "gsr_image_loss_workspace")
        values = torch.empty(3, dtype=torch.float32, device=image.device)
        saved = torch.empty((3, C, H, W), dtype=torch.float32,
                            device=image.device) if need_saved else None
        ws = torch.empty(nbytes, dtype=torch.uint8, device=image.device)
        _lib.check(forward(ctypes.byref(_inputs(image, target, lambda_dssim)), values.data_ptr(),
                           saved.data_ptr() if need_saved else None, ws.data_ptr(),
                           _stream(image.device)), "gsr_image_loss")
    return values, saved


def image_loss_backward_native(image, target, lambda_dssim, saved, dL_dloss=None):
    """gsr_image_loss_backward by ctypes on torch's current stream -> dL_dimage [C, H, W];
    `dL_dloss` is a one-element float32 device tensor, or None for 1.0."""
    lib = _lib.load_library()
    backward = _lib.image_loss_fns(lib)[2]
    grad = torch.empty_like(image)
    with torch.cuda.device(image.device):
        _lib.check(backward(ctypes.byref(_inputs(image, target, lambda_dssim)), saved.data_ptr(),
                            None if dL_dloss is None else dL_dloss.data_ptr(), grad.data_ptr(),
                            _stream(image.device)), "gsr_image_loss_backward")
    return grad


def _forward(image, target, lam, need_saved):
    """(values, saved or None): through `_C`, under GSR_LIB (an A/B build) by ctypes."""
    if not _lib._native_shares_library():
        return image_loss_native(image, target, lam, need_saved)
    from . import _C
    values, saved = _C.fused_image_loss(image, target, lam, need_saved)
    return values, (saved if need_saved else None)


def _backward(image, target, lam, saved, dL_dloss):
    if not _lib._native_shares_library():
        return image_loss_backward_native(image, target, lam, saved, dL_dloss)
    from . import _C
    return _C.fused_image_loss_backward(image, target, lam, saved, dL_dloss)


class _PhotometricLoss(torch.autograd.Function):
    """-> (loss, l1, ssim), 0-dim; l1 and ssim are not differentiable."""

    @staticmethod
    def forward(ctx, image, target, lam):
        values, saved = _forward(image, target, lam, True)
        ctx.save_for_backward(image, target, saved)
        ctx.lam = lam
        loss, l1, ssim = values.unbind(0)
        ctx.mark_non_differentiable(l1, ssim)
        return loss, l1, ssim

    @staticmethod
    def backward(ctx, grad_loss, _grad_l1, _grad_ssim):
        image, target, saved = ctx.saved_tensors
        g = grad_loss.detach().to(torch.float32).reshape(1).contiguous()
        return _backward(image, target, ctx.lam, saved, g), None, None


def _checked(image, target, lam):
    if not (torch.is_tensor(image) and torch.is_tensor(target)):
        raise ValueError("image and target must be tensors")
    if image.dim() != 3 or image.shape != target.shape:
        raise ValueError(f"image and target must have one shape (C, H, W), got "
                         f"{tuple(image.shape)} and {tuple(target.shape)}")
    if min(image.shape) < 1:
        raise ValueError(f"empty image {tuple(image.shape)}")
    if target.requires_grad:
        raise ValueError("target is a constant of the loss: it must not require a gradient")
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_dssim must be in [0, 1], got {lam}")
    if image.device != target.device:
        raise ValueError(f"image is on {image.device}, target on {target.device}")
    if image.device.type != "cuda":
        raise ValueError(f"image and target must be on a HIP device, not {image.device}: there "
                         "is no CPU fallback")
    return (image.to(torch.float32).contiguous(), target.detach().to(torch.float32).contiguous(),
            lam)


def photometric_loss(image, target, lambda_dssim=LAMBDA_DSSIM, return_parts=False):
    """(1 - lambda_dssim) * mean|image - target| + lambda_dssim * (1 - SSIM(image, target)) of
    two [C, H, W] images on a HIP device, as a 0-dim tensor differentiable with respect to
    `image`.  With `return_parts`: (loss, l1, ssim), the two parts detached.  Under `no_grad`,
    or for an `image` that requires no gradient, nothing is kept for a backward.  ValueError for
    shapes that differ or are not 3-D, tensors on different devices or not on a HIP device, and
    a `target` that requires a gradient.  Runs on torch's current stream."""
    image, target, lam = _checked(image, target, lambda_dssim)
    if torch.is_grad_enabled() and image.requires_grad:
        loss, l1, ssim = _PhotometricLoss.apply(image, target, lam)
    else:
        loss, l1, ssim = _forward(image.detach(), target, lam, False)[0].unbind(0)
    return (loss, l1, ssim) if return_parts else loss


def ssim(image, target):
    """SSIM(image, target) alone, a 0-dim tensor; not differentiable."""
    image, target, _ = _checked(image, target, 0.0)
    return _forward(image.detach(), target, 1.0, False)[0][2]
