"""Adaptive density control of a 3D Gaussian Splatting fit: upstream's densify_and_prune (clone
the small hot Gaussians, split the large hot ones in two, prune the transparent and the oversized)
over the tensors of a `SparseGaussianAdam`, planned and applied by HIP kernels
(gsr_densify_plan / gsr_densify_apply; include/gsr.h states the semantics, DESIGN.md §3p the
design).

    densification_stats(radii, means2D.grad, grad_accum, denom, max_radii2D)   # every iteration
    ...
    r = densify_and_prune(opt, grad_accum, denom, max_radii2D, max_grad=2e-4, min_opacity=0.005,
                          extent=scene_extent, max_screen_size=20, seed=iteration)
    xyz, scaling = r.params["xyz"], r.params["scaling"]         # the optimizer's new Parameters
    grad_accum, denom, max_radii2D = r.grad_accum, r.denom, r.max_radii2D       # fresh zeros [P']
    features = features[r.source_index.long()]                 # state that is not in the optimizer

The split samples come from Philox4x32-10 keyed by `seed` and counted by (source row, child): the
same seed gives the same bits, whatever ran before and on whatever stream.  The call synchronises
once, to read the four counts that size the outputs.

There is no fallback: without libgsr.so or a HIP device the calls raise.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .optim import _on_hip, _stream

ROLES = ("xyz", "scaling", "rotation", "opacity")
_ROLE_ID = dict(xyz=_lib.GSR_ROLE_XYZ, scaling=_lib.GSR_ROLE_SCALING,
                rotation=_lib.GSR_ROLE_ROTATION, opacity=_lib.GSR_ROLE_OPACITY)
_ROLE_M = dict(xyz=3, scaling=3, rotation=4, opacity=1)


class DensifyInputs(NamedTuple):
    """What both steps read besides the groups (gsr_densify_plan_inputs): contiguous device tensors
    and thresholds that are float32 values in the tensors' stored space."""
    grad_accum: torch.Tensor
    denom: torch.Tensor
    max_radii: Optional[torch.Tensor]   # int32 [P] or None
    scaling: torch.Tensor               # [P, 3]
    opacity: torch.Tensor               # [P] or [P, 1]
    thresholds: tuple                   # grad, scale split, opacity prune, scale prune
    radius_threshold: int               # <= 0 = off
    scale_space: int                    # _lib.GSR_SCALE_LINEAR / GSR_SCALE_LOG
    seed: int


class DensifyCounts(NamedTuple):
    n_kept: int
    n_clone: int
    n_split: int
    n_removed: int

    @property
    def total(self) -> int:
        return self.n_kept + self.n_clone + _lib.SPLIT_CHILDREN * self.n_split


class DensifyResult(NamedTuple):
    params: dict                        # group name -> the new nn.Parameter [P', ...]
    counts: DensifyCounts
    source_index: torch.Tensor          # int32 [P']: the source row of every new row
    grad_accum: torch.Tensor            # zeros, the old one's trailing shape
    denom: torch.Tensor
    max_radii2D: Optional[torch.Tensor]


def _f32(x: float) -> float:
    """A double rounded once to float32."""
    return float(np.float32(x))


def _log(x: float) -> float:
    return math.log(x) if x > 0.0 else -math.inf


def stored_thresholds(max_grad, min_opacity, extent, max_screen_size=None, percent_dense=0.01,
                      activated=False):
    """Upstream's arguments -> ((grad, scale split, opacity prune, scale prune), radius threshold)
    in the space the tensors are stored in, computed in double and rounded once to float32:
    log(percent_dense * extent), logit(min_opacity) and log(0.1 * extent) for raw tensors (log
    scales, logit opacities), the plain values for `activated` ones.  Without `max_screen_size`
    (None or 0, as upstream tests it) the screen-size and the world-size test are off."""
    split, world = percent_dense * extent, 0.1 * extent
    opacity = float(min_opacity)
    if not activated:
        split, world = _log(split), _log(world)
        opacity = (-math.inf if opacity <= 0.0 else math.inf if opacity >= 1.0
                   else math.log(opacity / (1.0 - opacity)))
    radius = 0
    if not max_screen_size:
        world = math.inf
    else:
        radius = min(int(math.floor(max_screen_size)), 2 ** 31 - 1)  # int r > x <=> r > floor(x)
    return (_f32(max_grad), _f32(split), _f32(opacity), _f32(world)), radius


def workspace_words(P: int) -> int:
    """gsr_densify_workspace(P) in int32 words."""
    ws_fn, _, _ = _lib.densify_fns(_lib.load_library())
    return (_lib.check(ws_fn(P), "gsr_densify_workspace") + 3) // 4


def _plan_inputs(inp: DensifyInputs, P_out=0, n_groups=0):
    t = inp.thresholds
    return _lib.GsrDensifyPlanInputs(
        inp.scaling.shape[0], P_out, inp.seed & (2 ** 64 - 1), n_groups, inp.scale_space, t[0],
        t[1], t[2], t[3], inp.radius_threshold, inp.grad_accum.data_ptr(), inp.denom.data_ptr(),
        None if inp.max_radii is None else inp.max_radii.data_ptr(), inp.scaling.data_ptr(),
        inp.opacity.data_ptr())


def _use_native(route):
    if route is None:
        return _lib._native_shares_library()
    if route not in ("_C", "ctypes"):
        raise ValueError(f"route must be None, '_C' or 'ctypes', got {route!r}")
    return route == "_C"


def _c_inputs(inp: DensifyInputs):
    dev = inp.scaling.device
    return (inp.grad_accum, inp.denom,
            torch.empty(0, dtype=torch.int32, device=dev) if inp.max_radii is None
            else inp.max_radii, inp.scaling, inp.opacity, list(inp.thresholds),
            inp.radius_threshold, inp.scale_space)


def plan(inp: DensifyInputs, workspace, counts, route=None):
    """gsr_densify_plan on torch's current stream: classify and scan into `workspace` (int32, at
    least workspace_words(P)) and the four `counts` (int32 [4], on the device).  Through `_C`, or
    by ctypes (under GSR_LIB, or with route="ctypes")."""
    if _use_native(route):
        from . import _C
        return _C.densify_plan(*_c_inputs(inp), workspace, counts)
    _, plan_fn, _ = _lib.densify_fns(_lib.load_library())
    dev = inp.scaling.device
    with torch.cuda.device(dev):
        _lib.check(plan_fn(ctypes.byref(_plan_inputs(inp)), workspace.data_ptr(),
                           counts.data_ptr(), _stream(dev)), "gsr_densify_plan")


def apply(inp: DensifyInputs, roles, src, dst, workspace, source_index, route=None):
    """gsr_densify_apply on torch's current stream.  `roles`: a role name or None per group;
    `src` / `dst`: (param, exp_avg, exp_avg_sq) per group, [P, ...] and [P', ...], the moments
    None for a tensor without; P' is `source_index`'s length."""
    n, P, P_out = len(src), inp.scaling.shape[0], source_index.numel()
    ids = [_lib.GSR_ROLE_NONE if r is None else _ROLE_ID[r] for r in roles]
    if _use_native(route):
        from . import _C
        has = [int(s[1] is not None) for s in src]
        pick = lambda groups, k: [g[0] if g[k] is None else g[k] for g in groups]  # noqa: E731
        return _C.densify_apply(*_c_inputs(inp), inp.seed & (2 ** 64 - 1), ids, has,
                                pick(src, 0), pick(src, 1), pick(src, 2), pick(dst, 0),
                                pick(dst, 1), pick(dst, 2), workspace, source_index)
    _, _, apply_fn = _lib.densify_fns(_lib.load_library())
    tables = []
    for groups, rows in ((src, P), (dst, P_out)):
        table = (_lib.GsrDensifyGroup * max(n, 1))()
        for i, (p, m, v) in enumerate(groups):
            M = p.numel() // rows if rows else src[i][0].numel() // P if P else 1
            table[i] = _lib.GsrDensifyGroup(M, ids[i], p.data_ptr(),
                                            None if m is None else m.data_ptr(),
                                            None if v is None else v.data_ptr())
        tables.append(table)
    dev = inp.scaling.device
    with torch.cuda.device(dev):
        _lib.check(apply_fn(ctypes.byref(_plan_inputs(inp, P_out, n)), tables[0], tables[1],
                            workspace.data_ptr(), source_index.data_ptr(), _stream(dev)),
                   "gsr_densify_apply")


def _group_tensor(group, name):
    if len(group["params"]) != 1:
        raise ValueError(f"densify_and_prune takes one tensor per param group, group {name!r} has "
                         f"{len(group['params'])}")
    p = group["params"][0]
    _on_hip(p, f"the parameter of group {name!r}")
    if p.dtype != torch.float32 or not p.is_contiguous():
        raise ValueError(f"the parameter of group {name!r} must be a contiguous float32 tensor, "
                         f"got {p.dtype}, contiguous = {p.is_contiguous()}")
    return p


def _statistic(t, what, P, dtype, device):
    _on_hip(t, what)
    if t.device != device:
        raise ValueError(f"{what} is on {t.device}, the parameters on {device}")
    if t.dtype != dtype or t.numel() != P:
        raise ValueError(f"{what} must hold {P} {dtype} values, got {t.numel()} {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return t


@torch.no_grad()
def densify_and_prune(optimizer, grad_accum, denom, max_radii2D=None, *, max_grad, min_opacity,
                      extent, max_screen_size=None, percent_dense=0.01, seed, roles=None,
                      activated=False):
    """Upstream's densify_and_prune on every tensor of `optimizer` (one [P, ...] tensor per param
    group, found by the group's "name") and its Adam moments.

    `roles` maps xyz / scaling / rotation / opacity to the names of the groups that hold them
    (default: those names).  Raw tensors (log scales, logit opacities) by default;
    `activated=True` for linear scales and opacities in [0, 1].  `max_screen_size` tests
    `max_radii2D` as the caller passes it (upstream zeroes it first, so its test never fires:
    None gives upstream's behaviour).  Every group is rebound to a new nn.Parameter [P', ...]; the
    optimizer's state moves with it (`step` kept, moments gathered: copied for kept rows, zero for
    clones and children; a group without state gets none).  -> DensifyResult.
    ValueError for a tensor that is not a contiguous float32 (int32 for max_radii2D) tensor on one
    HIP device, a wrong length, a missing or repeated group name."""
    names = dict(zip(ROLES, ROLES))
    for k, v in (roles or {}).items():
        if k not in names:
            raise ValueError(f"roles maps {ROLES}, not {k!r}")
        names[k] = v
    by_name = {}
    for group in optimizer.param_groups:
        name = group.get("name")
        if name is None:
            raise ValueError('densify_and_prune finds tensors by the param group\'s "name"; a '
                             "group has none")
        if name in by_name:
            raise ValueError(f"two param groups are named {name!r}")
        by_name[name] = group
    for role, name in names.items():
        if name not in by_name:
            raise ValueError(f"no param group named {name!r} (the {role} role); the groups are "
                             f"{sorted(by_name)}")
    if len(set(names.values())) != len(ROLES):
        raise ValueError(f"one group holds two roles: {names}")
    tensors = {name: _group_tensor(g, name) for name, g in by_name.items()}
    xyz = tensors[names["xyz"]]
    P, device = xyz.shape[0] if xyz.dim() else 0, xyz.device
    for name, p in tensors.items():
        if p.device != device:
            raise ValueError(f"parameters on {device} and {p.device} in one call")
        if p.dim() < 1 or p.shape[0] != P:
            raise ValueError(f"group {name!r} has shape {tuple(p.shape)}, expected {P} rows")
    for role, name in names.items():
        M = tensors[name].numel() // P if P else _ROLE_M[role]
        if M != _ROLE_M[role]:
            raise ValueError(f"group {name!r} ({role}) has {M} floats per row, expected "
                             f"{_ROLE_M[role]}")
    _statistic(grad_accum, "grad_accum", P, torch.float32, device)
    _statistic(denom, "denom", P, torch.float32, device)
    if max_radii2D is not None:
        _statistic(max_radii2D, "max_radii2D", P, torch.int32, device)
    thresholds, radius = stored_thresholds(max_grad, min_opacity, extent, max_screen_size,
                                           percent_dense, activated)
    inp = DensifyInputs(grad_accum, denom, max_radii2D, tensors[names["scaling"]],
                        tensors[names["opacity"]], thresholds, radius,
                        _lib.GSR_SCALE_LINEAR if activated else _lib.GSR_SCALE_LOG, int(seed))

    counts = DensifyCounts(0, 0, 0, 0)
    if P:
        workspace = torch.empty(workspace_words(P), dtype=torch.int32, device=device)
        counts_dev = torch.empty(4, dtype=torch.int32, device=device)
        plan(inp, workspace, counts_dev)
        counts = DensifyCounts(*counts_dev.tolist())  # the call's one synchronisation
    P_out = counts.total
    source_index = torch.empty(P_out, dtype=torch.int32, device=device)

    def moments(p):
        st = optimizer.state.get(p, {})
        if "exp_avg" not in st:
            return None, None
        for k in ("exp_avg", "exp_avg_sq"):
            m = st[k]
            if (m.device != device or m.dtype != torch.float32 or not m.is_contiguous() or
                    m.shape != p.shape):
                raise ValueError(f"the optimizer's {k} of a {tuple(p.shape)} parameter must be a "
                                 "contiguous float32 tensor of its shape on its device")
        return st["exp_avg"], st["exp_avg_sq"]

    def like(t):
        return None if t is None else torch.empty((P_out,) + tuple(t.shape[1:]),
                                                  dtype=t.dtype, device=device)

    src = {name: (p,) + moments(p) for name, p in tensors.items()}
    dst = {name: tuple(like(t) for t in s) for name, s in src.items()}
    if P_out:
        # every call carries the four roles; the other groups ride along, four to a call
        role_names = [names[r] for r in ROLES]
        others = [n for n in tensors if n not in role_names]
        room = _lib.MAX_PARAM_GROUPS - len(ROLES)
        for i in range(0, max(len(others), 1), room):
            part = role_names + others[i:i + room]
            apply(inp, list(ROLES) + [None] * (len(part) - len(ROLES)),
                  [src[n] for n in part], [dst[n] for n in part], workspace, source_index)

    new = {}
    for name, group in by_name.items():
        old = tensors[name]
        fresh = torch.nn.Parameter(dst[name][0], requires_grad=old.requires_grad)
        state = optimizer.state.pop(old, None)
        if state is not None and len(state):
            state = dict(state)
            if dst[name][1] is not None:
                state["exp_avg"], state["exp_avg_sq"] = dst[name][1], dst[name][2]
            optimizer.state[fresh] = state
        group["params"][0] = fresh
        new[name] = fresh

    def zeros(t):
        return None if t is None else torch.zeros((P_out,) + tuple(t.shape[1:]), dtype=t.dtype,
                                                  device=device)

    return DensifyResult(new, counts, source_index, zeros(grad_accum), zeros(denom),
                         zeros(max_radii2D))
