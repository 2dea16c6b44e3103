"""PLY loading through the native reader.

Drop-in for the reference's `util_gau.load_ply(path)` (util_gau.py:63-125): same return value
`(GaussianData, bounding_box, center)` with the same activated float32 arrays, parsed by the
C++ reader in libgsr.so (csrc/ply_loader.hip: memory-mapped, multi-threaded) instead of
plyfile and per-property numpy loops.  `device=` loads straight into HIP device tensors (the
`GaussianDataHIP` the renderer consumes) through pinned staging, without building the numpy
arrays first.

`save_ply` / `load_scene_ply` are the other end of a fit: the raw tensors (the dict of
`scene_from_point_cloud`, or the optimizer that holds them) as the PLY upstream's
`GaussianModel.save_ply` writes, byte for byte, and back with the bits that were saved
(csrc/ply_writer.hip).  The file is what `load_ply`, `HIPRenderer` and the viewer
open.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib
from .gaussian_data import GaussianData


def _probe(path: str) -> _lib.GsrPlyInfo:
    lib = _lib.load_library()
    info = _lib.GsrPlyInfo()
    _lib.check(lib.gsr_ply_probe(os.fsencode(path), ctypes.byref(info)), "gsr_ply_probe")
    return info


def _bbox_center(info: _lib.GsrPlyInfo):
    bbox = np.array([list(info.bbox_min), list(info.bbox_max)], dtype=np.float32)
    return bbox, np.array(list(info.center), dtype=np.float32)


def load_ply(path: str, device=None):
    """util_gau.load_ply: returns (gaussians, bounding_box (2, 3), center (3,)).

    device=None: a host `GaussianData` (numpy float32: xyz (P,3), rot (P,4), scale (P,3),
    opacity (P,1), sh (P,48)).  device="cuda:i" (or a torch.device): a `GaussianDataHIP` whose
    tensors are filled on that device; sh is (P, 16, 3) as the renderer reshapes it."""
    info = _probe(path)
    P = int(info.P)
    lib = _lib.load_library()
    if device is None:
        xyz = np.empty((P, 3), np.float32)
        rot = np.empty((P, 4), np.float32)
        scale = np.empty((P, 3), np.float32)
        opacity = np.empty((P, 1), np.float32)
        sh = np.empty((P, 48), np.float32)
        ptrs = [a.ctypes.data_as(ctypes.c_void_p) for a in (xyz, rot, scale, opacity, sh)]
        _lib.check(lib.gsr_ply_load(os.fsencode(path), ctypes.byref(info), *ptrs, 0, None),
                   "gsr_ply_load")
        bbox, center = _bbox_center(info)
        return GaussianData(xyz, rot, scale, opacity, sh), bbox, center

    import torch
    from .renderer import GaussianDataHIP
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("device must be a HIP device (torch 'cuda:i') or None")
    t = {k: torch.empty(shape, dtype=torch.float32, device=dev) for k, shape in
         (("xyz", (P, 3)), ("rot", (P, 4)), ("scale", (P, 3)), ("opacity", (P, 1)),
          ("sh", (P, 16, 3)))}
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_ply_load(os.fsencode(path), ctypes.byref(info),
                                    *[ctypes.c_void_p(t[k].data_ptr() if P else 0)
                                      for k in ("xyz", "rot", "scale", "opacity", "sh")],
                                    1, ctypes.c_void_p(stream)), "gsr_ply_load")
    bbox, center = _bbox_center(info)
    return GaussianDataHIP(t["xyz"], t["rot"], t["scale"], t["opacity"], t["sh"]), bbox, center


SCENE_NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
_ROW_SHAPE = {"xyz": (3,), "f_dc": (1, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
_COEFFS = (1, 4, 9, 16, 25)


def _scene_tensors(scene) -> dict:
    """{name: array or tensor} of a scene dict or of an optimizer whose groups carry the names."""
    if hasattr(scene, "param_groups"):
        found = {}
        for group in scene.param_groups:
            name = group.get("name")
            if name not in SCENE_NAMES:
                continue
            if name in found:
                raise ValueError(f"two param groups are named {name!r}")
            if len(group["params"]) != 1:
                raise ValueError(f"save_ply takes one tensor per param group, group {name!r} has "
                                 f"{len(group['params'])}")
            found[name] = group["params"][0]
        scene = found
    elif not isinstance(scene, dict):
        raise ValueError("save_ply takes a scene dict (xyz, f_dc, f_rest, opacity, scaling, "
                         f"rotation) or an optimizer whose param groups carry those names, not "
                         f"{type(scene).__name__}")
    for name in SCENE_NAMES:
        if name not in scene and name != "f_rest":
            raise ValueError(f"the scene has no {name!r}; it has {sorted(scene)}")
    return {name: scene[name] for name in SCENE_NAMES if scene.get(name) is not None}


def _checked_scene(scene):
    """(tensors by name, P, M, device): every tensor contiguous float32 of its stated shape, all on
    one HIP device (device = its torch.device) or all on the host (device = None)."""
    tensors = _scene_tensors(scene)
    devices, out = set(), {}
    P = None
    for name, t in tensors.items():
        if isinstance(t, np.ndarray):
            ok = t.dtype == np.float32 and t.flags["C_CONTIGUOUS"]
            devices.add(None)
        else:
            import torch
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a numpy array or a torch tensor, not "
                                 f"{type(t).__name__}")
            t = t.detach()
            ok = t.dtype == torch.float32 and t.is_contiguous()
            if t.device.type not in ("cpu", "cuda"):
                raise ValueError(f"{name} is on {t.device}: a HIP device or the CPU is needed")
            devices.add(None if t.device.type == "cpu" else t.device)
        shape = tuple(t.shape)
        if not ok:
            raise ValueError(f"{name} must be a contiguous float32 tensor, got {t.dtype} with "
                             f"shape {shape}")
        if name == "f_rest":
            good = len(shape) == 3 and shape[2] == 3
            want = "(P, M - 1, 3)"
        else:
            good = shape[1:] == _ROW_SHAPE[name] and len(shape) == 1 + len(_ROW_SHAPE[name])
            want = f"(P, {', '.join(map(str, _ROW_SHAPE[name]))})"
        if not good:
            raise ValueError(f"{name} has shape {shape}, expected {want}")
        if P is None:
            P = shape[0]
        elif shape[0] != P:
            raise ValueError(f"{name} has {shape[0]} rows, xyz has {P}")
        out[name] = t
    if len(devices) != 1:
        raise ValueError(f"the scene's tensors are on different devices: "
                         f"{sorted(map(str, devices))}")
    M = 1 + (out["f_rest"].shape[1] if "f_rest" in out else 0)
    if M not in _COEFFS:
        raise ValueError(f"f_rest has {M - 1} coefficients per channel: M = {M} is not "
                         "(degree + 1)^2 for a degree 0..4")
    return out, int(P), M, devices.pop()


def _address(t) -> int:
    return t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


def _c_scene(tensors: dict, P: int, M: int, Mo: int = 0, chunk_rows: int = 0):
    sc = _lib.GsrPlyScene(P=P, sh_coeffs=M, file_sh_coeffs=Mo, chunk_rows=chunk_rows)
    for name in SCENE_NAMES:
        t = tensors.get(name)
        setattr(sc, name, _address(t) if t is not None and P and t.shape[1] else None)
    return sc


def save_ply(path, scene, *, sh_degree=None, chunk_rows=None) -> int:
    """Write a fit's raw scene as upstream's `save_ply` does (x y z, zero normals, f_dc, f_rest
    channel-major, opacity, scale, rot; binary little endian) and return its row count P.

    `scene`: the dict of `scene_from_point_cloud` (tensors or `nn.Parameter`s; `f_rest` optional at
    degree 0), a dict of numpy arrays, or a `torch.optim.Optimizer` (a `SparseGaussianAdam`) whose
    param groups carry those names.  Tensors on a HIP device are packed there on torch's current
    stream and leave through two pinned staging slots of `chunk_rows` rows; host tensors and numpy
    arrays are packed on the host.  `sh_degree` above the scene's pads the file's f_rest columns
    with zeros (`sh_degree=3` makes a degree-0..2 scene a file `load_ply` accepts).  The file
    replaces `path` only once it is complete.

    ValueError: a missing or repeated name, a tensor that is not contiguous float32 of the stated
    shape, row counts that differ, mixed devices, an f_rest whose M is no square, an `sh_degree`
    below the scene's."""
    tensors, P, M, device = _checked_scene(scene)
    Mo = 0
    if sh_degree is not None:
        Mo = (int(sh_degree) + 1) ** 2
        if int(sh_degree) < 0 or Mo < M:
            raise ValueError(f"sh_degree {sh_degree} is below the scene's ({M} coefficients): a "
                             "file cannot drop coefficients")
        if Mo not in _COEFFS:
            raise ValueError(f"sh_degree {sh_degree} is not in 0..4")
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise ValueError(f"chunk_rows must be positive, got {chunk_rows}")
    lib = _lib.load_library()
    save = _lib.ply_scene_fns(lib)[0]
    sc = _c_scene(tensors, P, M, Mo, int(chunk_rows or 0))
    if device is None:
        _lib.check(save(os.fsencode(path), ctypes.byref(sc), 0, None), "gsr_ply_save")
        return P
    import torch
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        _lib.check(save(os.fsencode(path), ctypes.byref(sc), 1, ctypes.c_void_p(stream)),
                   "gsr_ply_save")
    return P


def load_scene_ply(path, device=None) -> dict:
    """The raw scene of a 3DGS PLY: {xyz (P,3), f_dc (P,1,3), f_rest (P,M-1,3), opacity (P,1),
    scaling (P,3), rotation (P,4)} with the file's values as float32 -- for a file `save_ply`
    wrote, the bits that were saved.  No activation (unlike `load_ply`), any SH degree 0..4.

    device=None: numpy arrays.  A HIP device: tensors on it, ready for `nn.Parameter` and
    `SparseGaussianAdam`."""
    if device is not None:
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("device must be a HIP device (torch 'cuda:i') or None")
    lib = _lib.load_library()
    _, probe, load = _lib.ply_scene_fns(lib)
    info = _lib.GsrPlyScene()
    _lib.check(probe(os.fsencode(path), ctypes.byref(info)), "gsr_ply_probe_scene")
    P, M = int(info.P), int(info.sh_coeffs)
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, M - 1, 3), "opacity": (P, 1),
              "scaling": (P, 3), "rotation": (P, 4)}
    if device is None:
        out = {k: np.empty(s, np.float32) for k, s in shapes.items()}
        sc = _c_scene(out, P, M)
        _lib.check(load(os.fsencode(path), ctypes.byref(sc), 0, None), "gsr_ply_load_scene")
        return out
    out = {k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items()}
    sc = _c_scene(out, P, M)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(load(os.fsencode(path), ctypes.byref(sc), 1, ctypes.c_void_p(stream)),
                   "gsr_ply_load_scene")
    return out
