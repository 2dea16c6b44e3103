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
alone, zero padded at the strip's edges, NOT the frame's loss restricted to the strip.  That is
`frame_loss_on_strip`: the strip's share of the frame's loss, from the strip and ten rendered
rows of each neighbour (`strips.exchange_halo`), over gsr_image_loss_window:

    color, radii = GaussianRasterizer(settings_with_tile_rows)(...)
    y0, r = strip_pixel_rows(layout[rank], H)
    above, below = exchange_halo(color.detach(), layout, H, rank)
    share = frame_loss_on_strip(color, target, (y0, y0 + r), above=above, below=below)
    share.backward(); reduce_gradients(grads)   # the frame's loss and its gradients, on N GPUs

There is no fallback: without libgsr.so or a HIP device the calls raise.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib

LAMBDA_DSSIM = 0.2  # 3D Gaussian Splatting's weight of the D-SSIM term
# Rendered rows of each neighbour a strip needs for the frame's loss and its gradient: the map at
# a pixel reads the image within 5 rows, the gradient at a pixel the map's partials within 5 rows
HALO_ROWS = 10
_APRON = 5


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


def _window(frame_H: int, row0: int, own) -> _lib.GsrLossWindow:
    return _lib.GsrLossWindow(int(frame_H), int(row0), int(own[0]), int(own[1]))


def apron_rows(frame_H: int, own) -> tuple[int, int]:
    """The frame rows [a0, a1) of a window's `saved`: the own rows +- 5, clipped to the frame."""
    return max(0, own[0] - _APRON), min(frame_H, own[1] + _APRON)


def image_loss_window_native(image, target, frame_H, row0, own, lambda_dssim=LAMBDA_DSSIM,
                             need_saved=False):
    """gsr_image_loss_window by ctypes on torch's current stream -> (values [3], the window's
    shares of loss, l1, ssim; saved [3, C, A, W] over the apron, or None without `need_saved`).
    `image` and `target` are the contiguous float32 band buffers [C, rows, W] whose row 0 is frame
    row `row0`; `own` = (own_begin, own_end) in frame rows."""
    lib = _lib.load_library()
    workspace, forward, _ = _lib.image_loss_window_fns(lib)
    C, _, W = image.shape
    inputs, win = _inputs(image, target, lambda_dssim), _window(frame_H, row0, own)
    with torch.cuda.device(image.device):
        nbytes = _lib.check(workspace(ctypes.byref(inputs), ctypes.byref(win)),
                            "gsr_image_loss_window_workspace")
        a0, a1 = apron_rows(frame_H, own)
        values = torch.empty(3, dtype=torch.float32, device=image.device)
        saved = torch.empty((3, C, a1 - a0, W), dtype=torch.float32,
                            device=image.device) if need_saved else None
        ws = torch.empty(nbytes, dtype=torch.uint8, device=image.device)
        _lib.check(forward(ctypes.byref(inputs), ctypes.byref(win), values.data_ptr(),
                           saved.data_ptr() if need_saved else None, ws.data_ptr(),
                           _stream(image.device)), "gsr_image_loss_window")
    return values, saved


def image_loss_window_backward_native(image, target, frame_H, row0, own, lambda_dssim, saved,
                                      dL_dloss=None):
    """gsr_image_loss_window_backward by ctypes on torch's current stream -> the frame loss's
    gradient on the own rows, [C, own_end - own_begin, W]."""
    lib = _lib.load_library()
    backward = _lib.image_loss_window_fns(lib)[2]
    C, _, W = image.shape
    inputs, win = _inputs(image, target, lambda_dssim), _window(frame_H, row0, own)
    with torch.cuda.device(image.device):
        grad = torch.empty((C, own[1] - own[0], W), dtype=torch.float32, device=image.device)
        _lib.check(backward(ctypes.byref(inputs), ctypes.byref(win), saved.data_ptr(),
                            None if dL_dloss is None else dL_dloss.data_ptr(), grad.data_ptr(),
                            _stream(image.device)), "gsr_image_loss_window_backward")
    return grad


def _window_forward(image, target, frame_H, row0, own, lam, need_saved):
    """(values, saved or None) of a window: through `_C`, under GSR_LIB by ctypes."""
    if not _lib._native_shares_library():
        return image_loss_window_native(image, target, frame_H, row0, own, lam, need_saved)
    from . import _C
    values, saved = _C.fused_image_loss_window(image, target, frame_H, row0, own[0], own[1], lam,
                                               need_saved)
    return values, (saved if need_saved else None)


def _window_backward(image, target, frame_H, row0, own, lam, saved, dL_dloss):
    if not _lib._native_shares_library():
        return image_loss_window_backward_native(image, target, frame_H, row0, own, lam, saved,
                                                 dL_dloss)
    from . import _C
    return _C.fused_image_loss_window_backward(image, target, frame_H, row0, own[0], own[1], lam,
                                               saved, dL_dloss)


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


class _FrameLossOnStrip(torch.autograd.Function):
    """-> the window's shares (loss, l1, ssim), 0-dim; `strip` is the graph's input, the band
    buffers (which hold the strip's values) are constants."""

    @staticmethod
    def forward(ctx, strip, band_image, band_target, frame_H, row0, own, lam):
        values, saved = _window_forward(band_image, band_target, frame_H, row0, own, lam, True)
        ctx.save_for_backward(band_image, band_target, saved)
        ctx.window = (frame_H, row0, own, lam)
        loss, l1, ssim = values.unbind(0)
        ctx.mark_non_differentiable(l1, ssim)
        return loss, l1, ssim

    @staticmethod
    def backward(ctx, grad_loss, _grad_l1, _grad_ssim):
        band_image, band_target, saved = ctx.saved_tensors
        frame_H, row0, own, lam = ctx.window
        g = grad_loss.detach().to(torch.float32).reshape(1).contiguous()
        grad = _window_backward(band_image, band_target, frame_H, row0, own, lam, saved, g)
        return grad, None, None, None, None, None, None


def halo_counts(rows, H: int) -> tuple[int, int]:
    """(a, b): the rows above and below the strip `rows` = (y0, y1) of a frame of H rows that
    `frame_loss_on_strip` needs: HALO_ROWS, or what the frame has."""
    return min(HALO_ROWS, rows[0]), min(HALO_ROWS, H - rows[1])


def _checked_strip(image, target, rows, above, below, lam):
    """The band buffers of a strip -> (strip float32, band image, band target, row0, lam)."""
    if not (torch.is_tensor(image) and torch.is_tensor(target)):
        raise ValueError("image and target must be tensors")
    if image.dim() != 3 or target.dim() != 3:
        raise ValueError(f"image must be (C, rows, W) and target (C, H, W), got "
                         f"{tuple(image.shape)} and {tuple(target.shape)}")
    C, r, W = image.shape
    H = target.shape[1]
    if (target.shape[0], target.shape[2]) != (C, W) or min(C, W, H) < 1:
        raise ValueError(f"image {tuple(image.shape)} and target {tuple(target.shape)} must share "
                         "C >= 1 and W >= 1, and the frame must have rows")
    try:
        y0, y1 = (int(v) for v in rows)
    except (TypeError, ValueError):
        raise ValueError(f"rows must be (y0, y1), got {rows!r}") from None
    if not 0 <= y0 <= y1 <= H:
        raise ValueError(f"rows {(y0, y1)} are not inside the frame's [0, {H})")
    if y1 - y0 != r:
        raise ValueError(f"image has {r} rows, rows {(y0, y1)} are {y1 - y0}")
    if target.requires_grad:
        raise ValueError("target is a constant of the loss: it must not require a gradient")
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_dssim must be in [0, 1], got {lam}")
    parts = []
    a, b = halo_counts((y0, y1), H) if r else (0, 0)  # an empty strip has no neighbours to read
    for name, halo, n in zip(("above", "below"), (above, below), (a, b)):
        if halo is None:
            if n:
                raise ValueError(f"`{name}` must hold the {n} rendered rows next to the strip")
            continue
        if not torch.is_tensor(halo) or tuple(halo.shape) != (C, n, W):
            raise ValueError(f"`{name}` must be ({C}, {n}, {W}), got "
                             f"{tuple(halo.shape) if torch.is_tensor(halo) else halo!r}")
        if halo.requires_grad:
            raise ValueError(f"`{name}` is a constant of the loss (the neighbour differentiates "
                             "its own rows): it must not require a gradient")
        if halo.device != image.device:
            raise ValueError(f"image is on {image.device}, `{name}` on {halo.device}")
        parts.append((name, halo.to(torch.float32)))
    if image.device != target.device:
        raise ValueError(f"image is on {image.device}, target on {target.device}")
    if image.device.type != "cuda":
        raise ValueError(f"image and target must be on a HIP device, not {image.device}: there "
                         "is no CPU fallback")
    strip = image.to(torch.float32)
    if r == 0:
        return strip, None, None, y0, lam
    halos = dict(parts)
    band = [t for t in (halos.get("above"), strip.detach(), halos.get("below")) if t is not None]
    band_image = torch.cat(band, dim=1) if len(band) > 1 else band[0].contiguous()
    band_target = target.detach().to(torch.float32)[:, y0 - a:y1 + b].contiguous()
    return strip, band_image, band_target, y0 - a, lam


def frame_loss_on_strip(image, target, rows, *, above=None, below=None,
                        lambda_dssim=LAMBDA_DSSIM, return_parts=False):
    """The share of the FRAME's loss that the rendered rows `rows` = (y0, y1) carry: with the
    shares of a partition of the frame's rows added up (over the ranks), `photometric_loss` of
    the whole frame, and after `backward` on every share `image.grad` is the frame loss's
    gradient on these rows -- not the loss of the strip taken alone, which pads every seam.

    `image` [C, y1 - y0, W] is the strip as rendered (`tile_rows=`), the only differentiable
    input; `target` [C, H, W] is the whole frame's; `above` and `below` are the rendered frame
    rows [y0 - a, y0) and [y1, y1 + b), a = min(HALO_ROWS, y0), b = min(HALO_ROWS, H - y1)
    (`strips.exchange_halo`), constants like `target`, None only where the count is 0.  Returns
    the share of the loss, 0-dim; with `return_parts` the three shares (loss, l1, ssim):
    l1 = sum_own|d| / N, ssim = sum_own map / N, loss = (1 - lambda) l1 + lambda (n_own / N -
    ssim), N = C H W.  The gradient is that of the SUM of the shares under one upstream
    gradient: it includes the terms of map pixels within 5 rows that a neighbour sums.  An empty
    strip (y0 == y1) has the share 0 and reads no halo.

    Under `no_grad`, or for an `image` that requires no gradient, nothing is kept for a backward.
    The band buffers are assembled with one concatenation (above, strip, below) and one
    contiguous slice of the target: a copy of (y1 - y0 + a + b) rows of each, about the traffic
    of one more read and write of the strip pair, small beside the kernels' own.  ValueError for
    shapes that do not fit, `rows` outside the frame or not the image's, halos of another row
    count than (a, b), a `target` or halo that requires a gradient, tensors on different devices
    or not on a HIP device.  Runs on torch's current stream."""
    strip, band_image, band_target, row0, lam = _checked_strip(image, target, rows, above, below,
                                                               lambda_dssim)
    H, own = int(target.shape[1]), (int(rows[0]), int(rows[1]))
    if band_image is None:  # an empty strip: a zero share that still carries the graph
        zero = strip.sum()
        parts = (zero, zero.detach(), zero.detach())
    elif torch.is_grad_enabled() and strip.requires_grad:
        parts = _FrameLossOnStrip.apply(strip, band_image, band_target, H, row0, own, lam)
    else:
        parts = _window_forward(band_image, band_target, H, row0, own, lam, False)[0].unbind(0)
    return tuple(parts) if return_parts else parts[0]


def ssim(image, target):
    """SSIM(image, target) alone, a 0-dim tensor; not differentiable."""
    image, target, _ = _checked(image, target, 0.0)
    return _forward(image.detach(), target, 1.0, False)[0][2]
