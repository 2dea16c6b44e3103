"""GPU: the three autograd Functions by both of their paths -- the `_C` extension and ctypes (the
GSR_LIB A/B path, taken here on the same context by switching `_lib._native_shares_library`) -- on
the two scenes of aa_scenes that exercise both input forms, partial tiles and the antialiasing floor.

  forward    every returned tensor bit-equal between the two paths and to rasterize_gaussians_native
             with the matching extras / antialiasing
  gradients  each path by itself within the bound of the mode's existing `_C`-path test: with
             antialiasing aa_reference and its bounds (test_gpu_antialiasing.test_backward_autograd);
             without, grad_reference (colour), plane_grad_reference (planes) and, for the camera's
             three, camera_grad_reference, each with its own bounds (test_gpu_backward,
             test_gpu_plane_gradients, test_gpu_camera_gradients).  The sums are float atomics, so the
             two paths are not compared bit for bit.
  dropped work  an antialiased frame renders the same image with and without depth_maps, and an
             antialiased backward meets the same reference and bound with and without the camera.
"""
import numpy as np
import pytest
import torch

import aa_reference as ar
import aa_scenes
import camera_grad_reference as cg
import grad_reference as gr
import plane_grad_reference as pg
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import (PLANE_NAMES, GaussianRasterizationSettings,
                                                    GaussianRasterizer,
                                                    rasterize_gaussians_native)
from gpu_helpers import to_dev
from test_gpu_antialiasing import _aa_forward, _args, _assert_close, _bits, _plain_forward
from test_gpu_antialiasing import _reference as _aa_reference
from test_gpu_backward import END_TO_END

pytestmark = pytest.mark.gpu

SCENES = ("subpixel", "floor")
MODES = ("colour", "planes", "camera")
_ref_cache = {}


def _run(sc, gpu, mode, aa, depth_maps=None):
    """One forward and backward through GaussianRasterizer under the mode's loss: (the outputs as
    numpy arrays, the gradients as float64 by their gsr_gradients names)."""
    s, a = sc["s"], _args(sc, gpu)
    depth_maps = mode != "colour" if depth_maps is None else depth_maps
    leaves = dict(means3D=a["means3D"], opacities=a["opacities"], shs=a["sh"],
                  colors_precomp=a["colors"], scales=a["scales"], rotations=a["rotations"],
                  cov3D_precomp=a["cov6"])
    for v in leaves.values():
        if v is not None:
            v.requires_grad_(True)
    means2D = torch.zeros_like(a["means3D"], requires_grad=True)
    cam = [a["view"], a["proj"], a["campos"]]
    if mode == "camera":
        for t in cam:
            t.requires_grad_(True)
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], a["bg"], s["scale_modifier"], cam[0], cam[1],
        s["sh_degree"], cam[2], False, False, depth_maps=depth_maps, antialiasing=aa)
    out = GaussianRasterizer(rs)(means2D=means2D, **leaves)
    assert len(out) == (5 if depth_maps else 2)
    dL, dLp = ar.loss_gradients(sc, "combined" if depth_maps else "colour")
    total = (out[0] * to_dev(dL, gpu)).sum()
    if dLp is not None:
        total = total + sum((out[2 + i] * to_dev(dLp[i], gpu)).sum() for i in range(3))
    total.backward()
    grad = lambda t: None if t is None or t.grad is None else t.grad.cpu().numpy().astype(np.float64)  # noqa: E731
    got = dict(dL_dmeans3D=grad(leaves["means3D"]), dL_dmeans2D=grad(means2D),
               dL_dopacity=grad(leaves["opacities"]), dL_dscales=grad(leaves["scales"]),
               dL_drotations=grad(leaves["rotations"]), dL_dsh=grad(leaves["shs"]),
               dL_dcov3D=grad(leaves["cov3D_precomp"]), dL_dcolors=grad(leaves["colors_precomp"]))
    if mode == "camera":
        got.update(dL_dviewmatrix=grad(cam[0]), dL_dprojmatrix=grad(cam[1]), dL_dcampos=grad(cam[2]))
        if sc["colors"] is not None:  # (no SH: nothing reads campos)
            got.pop("dL_dcampos")
    return ([t.detach().cpu().numpy() for t in out], {k: v for k, v in got.items() if v is not None})


def _both_paths(sc, gpu, monkeypatch, mode, aa, depth_maps=None):
    """_run through `_C`, then by ctypes on the same context."""
    _lib.context(gpu.index or 0)  # (slot 0 is the extension's, whichever path renders)
    by_c = _run(sc, gpu, mode, aa, depth_maps)
    with monkeypatch.context() as m:
        m.setattr(_lib, "_native_shares_library", lambda: False)
        by_ctypes = _run(sc, gpu, mode, aa, depth_maps)
    return {"_C": by_c, "ctypes": by_ctypes}


def _plain_reference(sc, gpu, mode):
    """The float64 references of the plain backward's tests on the plain forward's lists: the
    Gaussians' (grad_reference under the colour loss, plane_grad_reference under the combined one)
    and, in the camera mode, camera_grad_reference for the camera's three."""
    key = (sc["name"], mode)
    if key not in _ref_cache:
        fwd = _plain_forward(sc, gpu)
        lists = (fwd["ranges"].view(np.uint32), fwd["point_list"].view(np.uint32))
        if mode == "colour":
            _ref_cache[key] = (gr.scene_gradients(sc, lists, fwd["radii"], sc["dL"]), None)
        else:
            dL, dLp = ar.loss_gradients(sc, "combined")
            _ref_cache[key] = (pg.scene_gradients(sc, lists, fwd["radii"], dL, dLp),
                               cg.scene_gradients(sc, lists, fwd["radii"], dL, dLp)
                               if mode == "camera" else None)
    return _ref_cache[key]


def _assert_plain_close(got, sc, gpu, mode, what):
    ref, cam_ref = _plain_reference(sc, gpu, mode)
    bound = gr.bound if mode == "colour" else pg.bound
    bad = []
    for name, key in END_TO_END:
        if key in ref and name in got:
            e = gr.rel_err(got[name].reshape(ref[key].shape), ref[key])
            print(f"{what}: e[{key}] = {e:.3e}  (bound {bound(key):.1e})")
            if not e <= bound(key):
                bad.append(f"{what}: e[{key}] = {e:.3e} > {bound(key):.1e}")
    for n in cg.CAMERA if cam_ref is not None else ():
        if "dL_d" + n in got:
            e = cg.cam_err(got["dL_d" + n].reshape(-1)[:len(cam_ref[n])], cam_ref, n)
            print(f"{what}: e[{n}] = {e:.3e}  (bound {cg.bound(n):.1e})")
            if not e <= cg.bound(n):
                bad.append(f"{what}: e[{n}] = {e:.3e} > {cg.bound(n):.1e}")
    assert not bad, bad


@pytest.mark.parametrize("aa", (False, True))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_both_paths(name, mode, aa, gpu, monkeypatch):
    sc = aa_scenes.get(name)
    runs = _both_paths(sc, gpu, monkeypatch, mode, aa)
    # the forward: the two paths, and the native entry with the matching arguments
    a = _args(sc, gpu)
    extras = PLANE_NAMES if mode != "colour" else ()
    res = rasterize_gaussians_native(
        a["bg"], a["means3D"], a["colors"], a["opacities"], a["scales"], a["rotations"], a["mod"],
        a["cov6"], a["view"], a["proj"], a["tx"], a["ty"], sc["H"], sc["W"], a["sh"], a["deg"],
        a["campos"], False, False, extras=extras, antialiasing=aa)
    want = [res.color, res.radii] + [res.extras[n] for n in extras]
    for path, (out, _) in runs.items():
        assert len(out) == len(want)
        for i, (x, y) in enumerate(zip(out, want)):
            np.testing.assert_array_equal(_bits(x), _bits(y.cpu().numpy()),
                                          err_msg=f"{name}/{mode}/aa={aa}/{path}: output {i}")
    # the gradients: each path by itself
    for path, (_, got) in runs.items():
        what = f"{name}/{mode}/aa={aa}/{path}"
        assert (got["dL_dmeans2D"][:, 2] == 0).all()
        if aa:
            ref = _aa_reference(sc, gpu, "colour" if mode == "colour" else "combined")
            _assert_close(got, ref, what)
        else:
            _assert_plain_close(got, sc, gpu, mode, what)


def test_dropped_work_changes_nothing(gpu, monkeypatch):
    """An antialiased frame without depth_maps renders no planes, and an antialiased backward
    without a camera gradient does not run the camera's kernels: the image has the bits of the
    frame with depth_maps, and the eight per-Gaussian gradients meet the reference and the bound
    they meet with the camera."""
    sc = aa_scenes.get("subpixel")
    ref = _aa_reference(sc, gpu, "combined")
    for path, (out, got) in _both_paths(sc, gpu, monkeypatch, "camera", True).items():
        with_planes = out
        _assert_close(got, ref, f"with the camera/{path}")
    for path, (out, got) in _both_paths(sc, gpu, monkeypatch, "planes", True).items():
        assert not any(k in got for k in ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"))
        _assert_close(got, ref, f"without the camera/{path}")
    for path, (out, _) in _both_paths(sc, gpu, monkeypatch, "colour", True).items():
        assert len(out) == 2
        np.testing.assert_array_equal(_bits(out[0]), _bits(with_planes[0]), err_msg=path)
        np.testing.assert_array_equal(_bits(out[0]), _bits(_aa_forward(sc, gpu)["color"]))
