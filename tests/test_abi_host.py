"""CPU: the C-ABI library loads and exports every symbol include/gsr.h declares, its struct
layouts agree with the ctypes mirrors, and the host-side API validates like upstream."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer, rasterize_gaussians_native)
from gaussiansplattingviewer_amd.strips import strip_rows, strip_pixel_rows

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gsr.h")


def _header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(gsr_[a-z_]+)\s*\(", src))


def test_library_exports_every_declared_symbol():
    lib = _lib.load_library()
    declared = _header_functions()
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.gsr_abi_version() == _lib.ABI_VERSION
    assert _lib.stage_names() == ["preprocess", "depth_sort", "scan", "duplicate", "tile_sort",
                                  "ranges", "blend", "color"]


def test_option_ids_match_header():
    """The GSR_OPT_* ids of include/gsr.h are the ones _lib exposes (ABI 2: six options -- the
    frame graphs' id 14 and the second stream's id 15 added in round 5 -- ids 10 and 12 of ABI 1
    retired)."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ids = {k: int(v) for k, v in re.findall(r"\b(GSR_OPT_[A-Z_]+)\s*=\s*(\d+)", src)}
    mine = {k: getattr(_lib, k) for k in dir(_lib) if k.startswith("GSR_OPT_")}
    assert ids == mine and len(ids) <= 6
    assert 10 not in ids.values() and 12 not in ids.values()


def test_library_is_gfx950_code_object():
    """The embedded device code object targets gfx950 (the MI355X) and nothing else."""
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    for other in (b"--gfx942", b"--gfx90a", b"--gfx1100"):
        assert other not in data


def test_struct_layouts_match_header(tmp_path):
    """Compile a probe against include/gsr.h with gcc and compare offsets with ctypes."""
    probe = tmp_path / "probe.c"
    fields = {
        "gsr_gaussians": [f for f, _ in _lib.GsrGaussians._fields_],
        "gsr_raster_settings": [f for f, _ in _lib.GsrRasterSettings._fields_],
        "gsr_outputs": [f for f, _ in _lib.GsrOutputs._fields_],
    }
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsr.h"', "int main(void){"]
    for st, fs in fields.items():
        lines.append(f'printf("{st} size %zu\\n", sizeof({st}));')
        for f in fs:
            lines.append(f'printf("{st} {f} %zu\\n", offsetof({st}, {f}));')
    lines.append("return 0;}")
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(probe), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l}
    for st, cls in [("gsr_gaussians", _lib.GsrGaussians),
                    ("gsr_raster_settings", _lib.GsrRasterSettings),
                    ("gsr_outputs", _lib.GsrOutputs)]:
        assert got[(st, "size")] == ctypes.sizeof(cls), st
        for f, _ in cls._fields_:
            assert got[(st, f)] == getattr(cls, f).offset, (st, f)


def _settings(H=64, W=64):
    eye = torch.eye(4)
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=0.5, tanfovy=0.5,
                                         bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=eye,
                                         projmatrix=eye, sh_degree=0, campos=torch.zeros(3),
                                         prefiltered=False, debug=False)


def test_rasterizer_argument_checks_match_upstream():
    r = GaussianRasterizer(_settings())
    x = torch.zeros(4, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(means3D=x, means2D=None, opacities=torch.ones(4, 1), shs=None, colors_precomp=None,
          scales=torch.ones(4, 3), rotations=torch.ones(4, 4))
    with pytest.raises(Exception, match="excatly one of either SHs"):
        r(means3D=x, means2D=None, opacities=torch.ones(4, 1), shs=torch.ones(4, 1, 3),
          colors_precomp=torch.ones(4, 3), scales=torch.ones(4, 3), rotations=torch.ones(4, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=x, means2D=None, opacities=torch.ones(4, 1), shs=torch.ones(4, 1, 3),
          scales=torch.ones(4, 3), rotations=None)
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=x, means2D=None, opacities=torch.ones(4, 1), shs=torch.ones(4, 1, 3),
          scales=torch.ones(4, 3), rotations=torch.ones(4, 4), cov3D_precomp=torch.ones(4, 6))


def test_debug_forward_leaves_a_snapshot(tmp_path, monkeypatch):
    """debug=True (upstream __init__.py): the arguments are copied to the host before the
    forward, and a forward that raises writes them to snapshot_fw.dump in the working directory
    (the file the reference ignores, /root/reference/.gitignore:7), then re-raises.  Without
    debug nothing is written.  The dump loads with weights_only=True."""
    from gaussiansplattingviewer_amd import rasterizer
    monkeypatch.chdir(tmp_path)
    x = torch.arange(16, dtype=torch.float32).reshape(4, 4)  # (P, 4): the extension refuses it
    bad = dict(means3D=x, means2D=None, opacities=torch.ones(4, 1), shs=torch.ones(4, 1, 3),
               scales=torch.ones(4, 3), rotations=torch.ones(4, 4))
    with pytest.raises(RuntimeError, match=r"means3D must have dimensions \(num_points, 3\)"):
        GaussianRasterizer(_settings())(**bad)
    assert not (tmp_path / rasterizer.SNAPSHOT_FILE).exists()
    with pytest.raises(RuntimeError, match=r"means3D must have dimensions \(num_points, 3\)"):
        GaussianRasterizer(_settings()._replace(debug=True))(**bad)
    args = torch.load(tmp_path / rasterizer.SNAPSHOT_FILE, weights_only=True)
    assert len(args) == 19  # _C.rasterize_gaussians' arguments, in upstream's order
    assert torch.equal(args[1], x) and args[1].device.type == "cpu"
    assert args[12:14] == (64, 64) and args[15] == 0 and args[18] is True
    assert args[2].numel() == 0 and torch.equal(args[14], torch.ones(4, 1, 3))  # colors absent


def test_native_radii_optional_only_on_strips():
    with pytest.raises(RuntimeError, match="radii=False needs tile_rows"):
        rasterize_gaussians_native(torch.zeros(3), torch.zeros(4, 3), None, torch.ones(4, 1),
                                   torch.ones(4, 3), torch.ones(4, 4), 1.0, None, torch.eye(4),
                                   torch.eye(4), 0.5, 0.5, 8, 8, None, 0, torch.zeros(3), False,
                                   False, radii=False)


def test_native_rejects_bad_means_shape():
    with pytest.raises(RuntimeError, match=r"means3D must have dimensions \(num_points, 3\)"):
        rasterize_gaussians_native(torch.zeros(3), torch.zeros(4, 4), None, torch.ones(4, 1),
                                   None, None, 1.0, None, torch.eye(4), torch.eye(4), 1.0, 1.0,
                                   8, 8, torch.zeros(4, 1, 3), 0, torch.zeros(3), False, False)


def test_no_cpu_fallback():
    """Host tensors never get rendered on the CPU: the product path refuses them."""
    with pytest.raises(RuntimeError, match="device"):
        rasterize_gaussians_native(torch.zeros(3), torch.zeros(4, 3), None, torch.ones(4, 1),
                                   torch.ones(4, 3), torch.ones(4, 4), 1.0, None, torch.eye(4),
                                   torch.eye(4), 1.0, 1.0, 8, 8, torch.zeros(4, 1, 3), 0,
                                   torch.zeros(3), False, False)


@pytest.mark.parametrize("gy,world", [(68, 1), (68, 2), (68, 8), (135, 8), (30, 4), (5, 8)])
def test_strip_rows_partition(gy, world):
    rows = [strip_rows(gy, world, r) for r in range(world)]
    assert rows[0][0] == 0 and rows[-1][1] == gy
    for (a0, a1), (b0, b1) in zip(rows, rows[1:]):
        assert a1 == b0
    sizes = [b - a for a, b in rows]
    assert max(sizes) - min(sizes) <= 1
    H = gy * 16 - 7
    covered = sum(strip_pixel_rows(r, H)[1] for r in rows)
    assert covered == H


def test_torch_extension_binds_upstream_entry_points():
    """`_C` is the compiled PyTorch extension (_native.so, csrc/torch_ext.cpp) over libgsr.so:
    upstream's two entry points with their argument counts, the same ABI as the ctypes
    loader, and upstream's input checks (these fail before any device call)."""
    from gaussiansplattingviewer_amd import _C, _native
    assert _C.rasterize_gaussians is _native.rasterize_gaussians
    assert _C.mark_visible is _native.mark_visible
    assert _native.__file__.endswith("_native.so")
    assert _native.abi_version() == _lib.load_library().gsr_abi_version() == _lib.ABI_VERSION
    sig = _native.rasterize_gaussians.__doc__.splitlines()[0]
    assert sig.startswith("rasterize_gaussians(") and sig.count("arg") == 19, sig
    assert _native.mark_visible.__doc__.splitlines()[0].count("arg") == 3
    e = torch.empty(0)
    with pytest.raises(RuntimeError, match=r"means3D must have dimensions \(num_points, 3\)"):
        _C.rasterize_gaussians(torch.zeros(3), torch.zeros(4, 4), e, torch.ones(4, 1), e, e, 1.0,
                               e, torch.eye(4), torch.eye(4), 0.5, 0.5, 8, 8, e, 0,
                               torch.zeros(3), False, False)
    with pytest.raises(RuntimeError, match="must be a device"):
        _C.rasterize_gaussians(torch.zeros(3), torch.zeros(4, 3), e, torch.ones(4, 1), e, e, 1.0,
                               e, torch.eye(4), torch.eye(4), 0.5, 0.5, 8, 8, e, 0,
                               torch.zeros(3), False, False)
    with pytest.raises(RuntimeError, match="must be a device"):
        _C.mark_visible(torch.zeros(4, 3), torch.eye(4), torch.eye(4))


def test_rasterizer_reaches_native_entry_with_upstream_args(monkeypatch):
    """GaussianRasterizer reaches `_C.rasterize_gaussians` through `_RasterizeGaussians`
    (upstream __init__.py's call chain) with upstream's argument order, absent inputs as empty
    tensors, and keeps (color, radii) of the 6-field return.  The native call is replaced here
    (no GPU in the CPU suite); the GPU suite runs the real one."""
    from gaussiansplattingviewer_amd import _C
    seen = {}

    def fake_native(*args):
        seen["args"] = args
        P = args[1].shape[0]
        H, W = args[12], args[13]
        u8 = torch.empty(0, dtype=torch.uint8)
        return 7, torch.zeros(3, H, W), torch.ones(P, dtype=torch.int32), u8, u8, u8

    monkeypatch.setattr(_C, "rasterize_gaussians", fake_native)
    P, H, W = 5, 4, 6
    xyz, op = torch.zeros(P, 3), torch.ones(P, 1)
    sc, rot, sh = torch.ones(P, 3), torch.ones(P, 4), torch.zeros(P, 16, 3)
    rs = GaussianRasterizationSettings(H, W, 0.5, 0.4, torch.zeros(3), 1.0, torch.eye(4),
                                       torch.eye(4), 3, torch.zeros(3), False, False)
    c2, r2 = GaussianRasterizer(rs)(means3D=xyz, means2D=None, opacities=op, shs=sh,
                                    colors_precomp=None, scales=sc, rotations=rot,
                                    cov3D_precomp=None)
    a = seen["args"]
    assert len(a) == 19 and a[1] is xyz and a[3] is op and a[4] is sc and a[5] is rot
    assert a[14] is sh and a[12:14] == (H, W) and a[15] == 3
    assert a[2].numel() == 0 and a[7].numel() == 0  # colors_precomp, cov3D_precomp absent
    assert tuple(c2.shape) == (3, H, W) and tuple(r2.shape) == (P,)


def _fake_C(monkeypatch, seen):
    """Replace the `_C` entries the Functions call by fakes that record their arguments and
    return tensors of the right shapes (no GPU in the CPU suite)."""
    from gaussiansplattingviewer_amd import _C

    def forward(name, n_args):
        def fake(*args):
            assert len(args) == n_args
            seen.setdefault(name, []).append(args)
            P, (H, W) = args[1].shape[0], args[12:14]
            planes = n_args == 22 and args[20]
            maps = [torch.full((H, W), float(i)) if planes else torch.empty(0) for i in range(3)]
            return (7, torch.zeros(3, H, W), torch.ones(P, dtype=torch.int32), *maps)
        return fake

    def backward(name, n_args, means3D_at, sh_at):
        def fake(*args):
            assert len(args) == n_args
            seen.setdefault(name, []).append(args)
            P, M = args[means3D_at].shape[0], args[sh_at].shape[1]
            g = tuple(torch.full(s, float(i)) for i, s in enumerate(
                ((P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, M, 3), (P, 3), (P, 4))))
            if n_args == 22 and name.endswith("_ext"):
                camera = args[20]
                g += tuple(torch.full(s, 9.0) if camera else torch.empty(0)
                           for s in ((4, 4), (4, 4), (3,)))
            return g
        return fake

    monkeypatch.setattr(_C, "rasterize_gaussians", forward("rasterize_gaussians", 19))
    monkeypatch.setattr(_C, "rasterize_gaussians_ext", forward("rasterize_gaussians_ext", 22))
    monkeypatch.setattr(_C, "rasterize_gaussians_backward",
                        backward("rasterize_gaussians_backward", 22, 1, 13))
    monkeypatch.setattr(_C, "rasterize_gaussians_backward_ext",
                        backward("rasterize_gaussians_backward_ext", 22, 1, 12))


@pytest.mark.parametrize("depth_maps,antialiasing,camera", [
    (False, False, False), (True, False, False), (False, True, False), (True, True, False),
    (False, False, True), (True, True, True)])
def test_functions_route_to_the_general_entries(depth_maps, antialiasing, camera, monkeypatch):
    """GaussianRasterizer's three Functions reach `_C` with the request spelt out: the general
    forward with (shading, planes, antialiasing) and the general backward with (camera,
    antialiasing), gradients that are None as empty tensors; a plain frame still reaches upstream's
    `_C.rasterize_gaussians` with its 19 arguments and upstream's backward."""
    seen = {}
    _fake_C(monkeypatch, seen)
    P, H, W = 5, 4, 6
    xyz, op = torch.zeros(P, 3, requires_grad=True), torch.ones(P, 1, requires_grad=True)
    sc, rot = torch.ones(P, 3, requires_grad=True), torch.ones(P, 4, requires_grad=True)
    sh = torch.zeros(P, 16, 3, requires_grad=True)
    view, campos = torch.eye(4, requires_grad=camera), torch.zeros(3)
    rs = GaussianRasterizationSettings(H, W, 0.5, 0.4, torch.zeros(3), 1.0, view, torch.eye(4), 3,
                                       campos, False, False, depth_maps=depth_maps,
                                       antialiasing=antialiasing)
    out = GaussianRasterizer(rs)(means3D=xyz, means2D=None, opacities=op, shs=sh,
                                 colors_precomp=None, scales=sc, rotations=rot,
                                 cov3D_precomp=None)
    assert len(out) == (5 if depth_maps else 2)
    if depth_maps or antialiasing:
        assert "rasterize_gaussians" not in seen
        (a,) = seen["rasterize_gaussians_ext"]
        assert a[19:] == (0, depth_maps, antialiasing)
        assert a[1] is xyz and a[14] is sh and a[12:14] == (H, W) and a[2].numel() == 0
    else:
        assert "rasterize_gaussians_ext" not in seen
        (a,) = seen["rasterize_gaussians"]
        assert len(a) == 19 and a[1] is xyz and a[14] is sh and a[7].numel() == 0
    if depth_maps:
        assert [float(out[2 + i].detach()[0, 0]) for i in range(3)] == [0.0, 1.0, 2.0]
    # the loss reads the image, and with depth_maps the first plane alone
    loss = out[0].sum() + (out[2].sum() if depth_maps else 0.0)
    loss.backward()
    if depth_maps or antialiasing or camera:
        assert "rasterize_gaussians_backward" not in seen
        (b,) = seen["rasterize_gaussians_backward_ext"]
        assert b[20:] == (camera, antialiasing)
        assert tuple(b[16].shape) == (3, H, W)
        assert tuple(b[17].shape) == ((H, W) if depth_maps else (0,))
        assert b[18].numel() == 0 and b[19].numel() == 0
        assert b[3] is not None and tuple(b[3].shape) == (P, 1) and b[15] is False
    else:
        assert "rasterize_gaussians_backward_ext" not in seen
        (b,) = seen["rasterize_gaussians_backward"]
        assert tuple(b[12].shape) == (3, H, W) and tuple(b[21].shape) == (P, 1)
    # the fake's i-th tensor is filled with i: (means2D, colors, opacity, means3D, cov3D, sh, ...)
    assert (xyz.grad == 3).all() and (op.grad == 2).all() and (sh.grad == 5).all()
    assert (sc.grad == 6).all() and (rot.grad == 7).all()
    if camera:
        assert tuple(view.grad.shape) == (4, 4) and (view.grad == 9).all()
    else:
        assert view.grad is None


ACCESSORS = {"forward_depth_fn": ("gsr_forward_depth",),
             "forward_surface_fn": ("gsr_forward_surface",),
             "backward_fn": ("gsr_backward",),
             "backward_planes_fn": ("gsr_backward_planes",),
             "backward_camera_fn": ("gsr_backward_camera",),
             "filtered_fns": ("gsr_forward_filtered", "gsr_backward_filtered")}


@pytest.mark.parametrize("accessor", sorted(ACCESSORS))
def test_additive_entry_accessors(accessor):
    """Each accessor returns the loaded library's own attribute(s), and says which symbol an
    older build lacks."""
    lib = _lib.load_library()
    symbols = ACCESSORS[accessor]
    got = getattr(_lib, accessor)(lib)
    want = tuple(getattr(lib, s) for s in symbols)
    assert (got if len(symbols) > 1 else (got,)) == want
    for fn in want:
        assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.c_void_p

    class Old:  # (a build of ABI 4 from before the additions)
        pass
    with pytest.raises(RuntimeError, match=f"no {symbols[0]}"):
        getattr(_lib, accessor)(Old())
