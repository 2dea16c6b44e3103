"""The parameter update of a 3D Gaussian Splatting fit: a visibility-masked ("sparse") Adam
whose step is ONE HIP kernel launch for all parameter tensors of the scene (gsr_adam_step), and
the densification statistics (gsr_densify_stats); include/gsr.h states the semantics, DESIGN.md
§3o the design.

    opt = SparseGaussianAdam([{"params": [xyz], "lr": 1.6e-4}, {"params": [f_dc], "lr": 2.5e-3},
                              ...], lr=0.0, eps=1e-15)
    color, radii = GaussianRasterizer(settings)(...)
    photometric_loss(color, target).backward()
    densification_stats(radii, means2D.grad, xyz_gradient_accum, denom, max_radii2D)
    opt.step(radii, N)

A Gaussian the frame culled (`radii <= 0`, or a False of a bool mask) keeps its parameters AND
its moments: neither is read or written, so the moments do not decay as torch.optim.Adam's would.
The step is elementwise (no atomics): the same inputs give the same bits, so with
`deterministic=True` and `photometric_loss` a whole fit iteration is bit-reproducible.

There is no fallback: without libgsr.so or a HIP device the calls raise.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib


def _stream(dev: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def adam_step_native(params, grads, exp_avgs, exp_avg_sqs, lrs, epss, mask, beta1, beta2,
                     bc1=1.0, bc2_sqrt=1.0):
    """gsr_adam_step by ctypes on torch's current stream, in place: 1..8 contiguous float32
    device tensors [P, M_i] with their gradients and moments; `mask` a bool / uint8 [P], an int32
    [P] (radii) or None."""
    adam_step, _ = _lib.optimizer_fns(_lib.load_library())
    n = len(params)
    P = params[0].shape[0]
    groups = (_lib.GsrParamGroup * max(n, 1))()
    for i in range(n):
        M = params[i].numel() // P if P else 1
        groups[i] = _lib.GsrParamGroup(M, lrs[i], epss[i], params[i].data_ptr(),
                                       grads[i].data_ptr(), exp_avgs[i].data_ptr(),
                                       exp_avg_sqs[i].data_ptr())
    s = _lib.GsrAdamSettings(P, n, beta1, beta2, bc1, bc2_sqrt, None, None)
    if mask is not None and mask.numel():
        if mask.dtype == torch.int32:
            s.radii = mask.data_ptr()
        else:
            s.visible = mask.data_ptr()
    with torch.cuda.device(params[0].device):
        _lib.check(adam_step(ctypes.byref(s), groups, _stream(params[0].device)),
                   "gsr_adam_step")


def densify_stats_native(radii, means2D_grad, grad_accum, denom, max_radii=None):
    """gsr_densify_stats by ctypes on torch's current stream, in place."""
    _, stats = _lib.optimizer_fns(_lib.load_library())
    inputs = _lib.GsrDensifyInputs(radii.numel(), radii.data_ptr(), means2D_grad.data_ptr(),
                                   grad_accum.data_ptr(), denom.data_ptr(),
                                   None if max_radii is None else max_radii.data_ptr())
    with torch.cuda.device(radii.device):
        _lib.check(stats(ctypes.byref(inputs), _stream(radii.device)), "gsr_densify_stats")


def _adam_step(params, grads, exp_avgs, exp_avg_sqs, lrs, epss, mask, beta1, beta2, bc1, bc2_sqrt):
    """Through `_C`, under GSR_LIB (an A/B build) by ctypes."""
    if not _lib._native_shares_library():
        return adam_step_native(params, grads, exp_avgs, exp_avg_sqs, lrs, epss, mask, beta1,
                                beta2, bc1, bc2_sqrt)
    from . import _C
    empty = torch.empty(0, dtype=torch.uint8, device=params[0].device)
    _C.fused_adam_step(params, grads, exp_avgs, exp_avg_sqs, lrs, epss,
                       empty if mask is None else mask, beta1, beta2, bc1, bc2_sqrt)


def _on_hip(t, what):
    if not torch.is_tensor(t):
        raise ValueError(f"{what} must be a tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{what} must be on a HIP device, not {t.device}: there is no CPU fallback")


def _mask(visibility, N, device):
    """None, or the mask as the kernel reads it: uint8 / bool [N] or int32 [N] on `device`."""
    if visibility is None:
        return None
    _on_hip(visibility, "visibility")
    if visibility.device != device:
        raise ValueError(f"visibility is on {visibility.device}, the parameters on {device}")
    if visibility.dtype not in (torch.bool, torch.uint8, torch.int32):
        raise ValueError(f"visibility must be bool, uint8 or int32 (radii), got {visibility.dtype}")
    if visibility.numel() != N:
        raise ValueError(f"visibility holds {visibility.numel()} values, expected N = {N}")
    return visibility.detach().reshape(-1).contiguous()


class SparseGaussianAdam(torch.optim.Adam):
    """torch.optim.Adam's state and param groups, upstream's SparseGaussianAdam's step: one
    tensor per param group, `step(visibility, N)` updates the rows of every tensor [N, ...] that
    `visibility` (a bool tensor, the rasterizer's int32 `radii`, or None for all) selects, all
    tensors in one kernel launch (calls of 8 for more than 8).  The state keys are torch's
    (`step`, `exp_avg`, `exp_avg_sq`, moments created zero on first use), so code that prunes or
    concatenates optimizer state works unchanged.  `bias_correction=False` is upstream's form;
    True is torch.optim.Adam's, the corrections computed in double from the state's step count.
    ValueError for weight_decay, amsgrad or maximize, and in `step` for a parameter that is not a
    contiguous float32 tensor on a HIP device or a mask of the wrong length."""

    def __init__(self, params, lr, eps, betas=(0.9, 0.999), bias_correction=False, **kwargs):
        for name in ("weight_decay", "amsgrad", "maximize"):
            if kwargs.get(name):
                raise ValueError(f"SparseGaussianAdam does not support {name}")
        super().__init__(params=params, lr=lr, eps=eps, betas=betas, **kwargs)
        for group in self.param_groups:
            for name in ("weight_decay", "amsgrad", "maximize"):
                if group.get(name):
                    raise ValueError(f"SparseGaussianAdam does not support {name}")
        self.bias_correction = bool(bias_correction)

    def _checked(self, group):
        if len(group["params"]) != 1:
            raise ValueError("SparseGaussianAdam takes one tensor per param group, got "
                             f"{len(group['params'])}")
        for name in ("weight_decay", "amsgrad", "maximize"):
            if group.get(name):
                raise ValueError(f"SparseGaussianAdam does not support {name}")
        p = group["params"][0]
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError("a parameter must be a contiguous float32 tensor, got "
                             f"{p.dtype}, contiguous = {p.is_contiguous()}")
        _on_hip(p, "a parameter")
        return p

    @torch.no_grad()
    def step(self, visibility=None, N=None):
        """One update of the rows `visibility` selects.  `N`: the number of Gaussians (the first
        dimension of the tensors that are updated; default: the first parameter's)."""
        todo = []
        for group in self.param_groups:
            p = self._checked(group)
            if N is None:
                N = p.shape[0] if p.dim() else 1
            if p.grad is None:
                continue
            if p.dim() < 1 or p.shape[0] != N:
                raise ValueError(f"a parameter of shape {tuple(p.shape)} in a step over N = {N} "
                                 "Gaussians")
            if p.grad.is_sparse:
                raise ValueError("SparseGaussianAdam takes dense gradients (the mask is the "
                                 "sparsity)")
            if todo and p.device != todo[0][1].device:
                raise ValueError(f"parameters on {todo[0][1].device} and {p.device} in one step")
            todo.append((group, p))
        if not todo or N == 0:
            return
        mask = _mask(visibility, N, todo[0][1].device)
        # groups that share their hyperparameters and step count share a call
        calls = {}
        for group, p in todo:
            state = self.state[p]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["step"] += 1
            beta1, beta2 = group["betas"]
            t = float(state["step"])
            calls.setdefault((float(beta1), float(beta2), t), []).append((group, p, state))
        for (beta1, beta2, t), members in calls.items():
            bc1 = bc2_sqrt = 1.0
            if self.bias_correction:
                bc1 = 1.0 - beta1 ** t
                bc2_sqrt = math.sqrt(1.0 - beta2 ** t)
            for i in range(0, len(members), _lib.MAX_PARAM_GROUPS):
                part = members[i:i + _lib.MAX_PARAM_GROUPS]
                _adam_step([p for _, p, _ in part], [p.grad.contiguous() for _, p, _ in part],
                           [s["exp_avg"] for _, _, s in part],
                           [s["exp_avg_sq"] for _, _, s in part],
                           [float(g["lr"]) for g, _, _ in part],
                           [float(g["eps"]) for g, _, _ in part], mask, beta1, beta2, bc1,
                           bc2_sqrt)


def densification_stats(radii, means2D_grad, grad_accum, denom, max_radii2D=None):
    """Upstream's add_densification_stats, in place, in one kernel: for every Gaussian with
    `radii > 0`, `grad_accum += |means2D_grad[:, :2]|`, `denom += 1` and, with `max_radii2D`
    (int32), `max_radii2D = max(max_radii2D, radii)`.  `radii` is the rasterizer's int32 [P],
    `means2D_grad` its [P, 3] gradient, the accumulators float32 [P] or [P, 1]."""
    for t, what in ((radii, "radii"), (means2D_grad, "means2D_grad"), (grad_accum, "grad_accum"),
                    (denom, "denom")) + (() if max_radii2D is None else
                                         ((max_radii2D, "max_radii2D"),)):
        _on_hip(t, what)
        if t.device != radii.device:
            raise ValueError(f"{what} is on {t.device}, radii on {radii.device}")
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous: it is updated in place")
    P = radii.numel()
    if radii.dtype != torch.int32 or (max_radii2D is not None and
                                      max_radii2D.dtype != torch.int32):
        raise ValueError("radii and max_radii2D must be int32")
    for t, what, n in ((means2D_grad, "means2D_grad", 3 * P), (grad_accum, "grad_accum", P),
                       (denom, "denom", P)):
        if t.dtype != torch.float32 or t.numel() != n:
            raise ValueError(f"{what} must hold {n} float32 values, got {t.numel()} {t.dtype}")
    if max_radii2D is not None and max_radii2D.numel() != P:
        raise ValueError(f"max_radii2D holds {max_radii2D.numel()} values, expected {P}")
    if P == 0:
        return
    with torch.no_grad():
        if not _lib._native_shares_library():
            return densify_stats_native(radii, means2D_grad, grad_accum, denom, max_radii2D)
        from . import _C
        _C.densification_stats(radii, means2D_grad, grad_accum, denom,
                               torch.empty(0, dtype=torch.int32, device=radii.device)
                               if max_radii2D is None else max_radii2D)
