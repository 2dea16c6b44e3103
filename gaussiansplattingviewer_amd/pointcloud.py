"""The start of a 3D Gaussian Splatting fit: the scene a point cloud gives (upstream's
`GaussianModel.create_from_pcd`), with the nearest-neighbour search of its initial scales in HIP
(gsr_knn_mean_dist2, upstream's `simple_knn._C.distCUDA2`; include/gsr.h states the semantics,
DESIGN.md §3t the design).

    xyz, rgb, _ = colmap.read_points3D_txt(colmap_dir)
    scene = scene_from_point_cloud(xyz, rgb, sh_degree=3)        # raw tensors on the HIP device
    params = {k: torch.nn.Parameter(v) for k, v in scene.items()}
    opt = SparseGaussianAdam([{"params": [p], "name": k, "lr": lr[k]} for k, p in params.items()])

The tensors are raw (log scales, logit opacities, unnormalised rotations), named as
`densify_and_prune`'s default roles name them.  The search is exact: `knn_mean_dist2` returns, bit
for bit, what a brute-force search over all pairs returns.

There is no fallback: without libgsr.so or a HIP device the calls raise.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .optim import _stream

SH_C0 = 0.28209479177387814


def _points(xyz, what="xyz"):
    if not torch.is_tensor(xyz):
        raise ValueError(f"{what} must be a tensor")
    if xyz.device.type != "cuda":
        raise ValueError(f"{what} must be on a HIP device, not {xyz.device}: there is no CPU "
                         "fallback")
    if xyz.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {xyz.dtype}")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{what} must have the shape (N, 3), got {tuple(xyz.shape)}")
    if not xyz.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return xyz


def workspace_bytes(N: int) -> int:
    """gsr_knn_workspace(N)."""
    ws_fn, _, _ = _lib.knn_fns(_lib.load_library())
    return _lib.check(ws_fn(N), "gsr_knn_workspace")


def knn_stages(xyz, dist2, workspace, n_stages=4):
    """gsr_knn_stages by ctypes on torch's current stream, into the caller's `dist2` (float32 [N])
    and `workspace` (a device tensor of at least workspace_bytes(N) bytes): the first `n_stages` of
    the search's four stages; 4 is gsr_knn_mean_dist2 itself.  No checks beyond the library's."""
    _, knn, stages = _lib.knn_fns(_lib.load_library())
    N, dev = xyz.shape[0], xyz.device
    with torch.cuda.device(dev):
        if n_stages == 4:
            rc = knn(xyz.data_ptr(), N, dist2.data_ptr(), workspace.data_ptr(), _stream(dev))
        else:
            rc = stages(xyz.data_ptr(), N, dist2.data_ptr(), workspace.data_ptr(), n_stages,
                        _stream(dev))
    _lib.check(rc, "gsr_knn_mean_dist2" if n_stages == 4 else "gsr_knn_stages")
    return dist2


def knn_mean_dist2(xyz, route=None):
    """The mean squared distance of every point of `xyz` (float32 [N, 3], contiguous, on a HIP
    device) to its min(3, N - 1) nearest neighbours -> float32 [N]: gsr_knn_mean_dist2 on torch's
    current stream, through `_C.distCUDA2`, or by ctypes (under GSR_LIB, or with route="ctypes").
    ValueError for a wrong dtype or shape, a non-contiguous or CPU tensor, and for a coordinate
    that is not finite (one device reduction and one readback)."""
    _points(xyz)
    if route not in (None, "_C", "ctypes"):
        raise ValueError(f"route must be None, '_C' or 'ctypes', got {route!r}")
    if not bool(torch.isfinite(xyz).all()):
        raise ValueError("xyz holds a coordinate that is not finite")
    if route == "_C" or (route is None and _lib._native_shares_library()):
        from . import _C
        return _C.distCUDA2(xyz)
    N = xyz.shape[0]
    dist2 = torch.empty(N, dtype=torch.float32, device=xyz.device)
    workspace = torch.empty(workspace_bytes(N), dtype=torch.uint8, device=xyz.device)
    return knn_stages(xyz, dist2, workspace)


def _to_device(a, device, what):
    if not torch.is_tensor(a):
        a = np.ascontiguousarray(a)
        a = torch.from_numpy(a if a.flags.writeable else a.copy())  # (torch wants it writable)
    t = a
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what} must have the shape (N, 3), got {tuple(t.shape)}")
    return t.to(device)


@torch.no_grad()
def scene_from_point_cloud(xyz, rgb, sh_degree=3, *, opacity=0.1, min_dist2=1e-7, device=None):
    """Upstream's create_from_pcd: the raw tensors of the scene a fit starts from.

    `xyz` (N, 3) and `rgb` (N, 3) are numpy arrays (what `colmap.read_points3D_txt` returns) or
    tensors; a uint8 `rgb` is divided by 255, a float one is taken as [0, 1].  `device`: a HIP
    device (default: a tensor `xyz`'s own when it is on one, else the current one).  -> a dict of
    float32 tensors on it, ready for nn.Parameter, `SparseGaussianAdam` and `densify_and_prune`:
      xyz      (N, 3)
      f_dc     (N, 1, 3)                        (rgb - 0.5) / 0.28209479177387814
      f_rest   (N, (sh_degree + 1)^2 - 1, 3)    0
      scaling  (N, 3)                           log(sqrt(max(dist2, min_dist2))), dist2 from
                                                `knn_mean_dist2`, the same on the three axes
      rotation (N, 4)                           (1, 0, 0, 0)
      opacity  (N, 1)                           log(opacity / (1 - opacity))
    ValueError for a wrong shape, a non-finite coordinate, sh_degree < 0, an opacity outside
    (0, 1) or a device that is not a HIP device."""
    if int(sh_degree) != sh_degree or sh_degree < 0:
        raise ValueError(f"sh_degree must be an integer >= 0, got {sh_degree!r}")
    if not 0.0 < opacity < 1.0:
        raise ValueError(f"opacity must lie in (0, 1), got {opacity!r}")
    if device is None:
        on_hip = torch.is_tensor(xyz) and xyz.device.type == "cuda"
        device = xyz.device if on_hip else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"device must be a HIP device, not {device}: there is no CPU fallback")
    points = _to_device(xyz, device, "xyz").to(torch.float32).contiguous()
    if points is xyz:
        points = points.clone()  # the scene owns its tensors
    colour = _to_device(rgb, device, "rgb")
    N = points.shape[0]
    if colour.shape[0] != N:
        raise ValueError(f"xyz has {N} rows, rgb {colour.shape[0]}")
    if colour.dtype == torch.uint8:
        # the 256 quotients, rounded once each on the host (a division by a scalar on the device
        # may be a multiplication by its reciprocal)
        levels = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0))
        colour = levels.to(device)[colour.long()]
    else:
        colour = colour.to(torch.float32)
    # (rgb - 0.5) / C0: the float32 difference, then the correctly rounded float32 quotient (the
    # quotient of two float32 values, taken in float64 and rounded once more, is that)
    f_dc = ((colour - 0.5).double() / float(np.float32(SH_C0))).float()
    dist2 = knn_mean_dist2(points)
    scaling = torch.log(torch.sqrt(torch.clamp_min(dist2, min_dist2)))[:, None].repeat(1, 3)
    rotation = torch.zeros((N, 4), dtype=torch.float32, device=device)
    rotation[:, 0] = 1.0
    return {
        "xyz": points,
        "f_dc": f_dc[:, None, :].contiguous(),
        "f_rest": torch.zeros((N, (int(sh_degree) + 1) ** 2 - 1, 3), dtype=torch.float32,
                              device=device),
        "scaling": scaling,
        "rotation": rotation,
        "opacity": torch.full((N, 1), math.log(opacity / (1.0 - opacity)), dtype=torch.float32,
                              device=device),
    }
