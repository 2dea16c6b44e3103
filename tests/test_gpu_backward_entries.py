"""GPU: gsr_backward_features is every backward entry below it.  Each entry is called by name, by
ctypes, with NULL for what the call does without, on the two scenes of test_gpu_function_paths.

  the same bits  deterministic = 1: gsr_backward_features (feat NULL), gsr_backward_strip and, on
                 the whole frame, gsr_backward_ordered give bit-equal gradients, plain, with the
                 planes, with the camera and with antialiasing; on tile row (1, 2) of the two, a
                 proper subset, the first two do.
  the atomic entries  gsr_backward, _planes, _camera and _filtered, and `_C`'s two calls
                 (upstream's entry, the top entry with NULLs), meet the float64 references within the
                 bounds their modes have in test_gpu_backward, test_gpu_plane_gradients,
                 test_gpu_camera_gradients and test_gpu_antialiasing (test_gpu_function_paths'
                 helpers): no tolerance of this file's own.
"""
import ctypes

import numpy as np
import pytest
import torch

import aa_reference as ar
import aa_scenes
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import _scene_structs
from gpu_helpers import to_dev
from test_gpu_antialiasing import _args, _assert_close, _bits
from test_gpu_antialiasing import _reference as _aa_reference
from test_gpu_function_paths import SCENES, _assert_plain_close, _run

pytestmark = pytest.mark.gpu

# entry -> how many of (planes, camera, filter, order, feat) it takes
ENTRIES = {"gsr_backward": 0, "gsr_backward_planes": 1, "gsr_backward_camera": 2,
           "gsr_backward_filtered": 3, "gsr_backward_ordered": 4, "gsr_backward_strip": 4,
           "gsr_backward_features": 5}
STRIP = (1, 2)  # of the scenes' two tile rows: pixel rows 16..24


def _call(entry, sc, gpu, planes=False, camera=False, aa=False, det=False, rows=None):
    """One call of `entry` under the scene's colour loss (with `planes` the combined one, on a
    strip both cut to its rows): the gradients by their struct names, float32 numpy arrays."""
    a = _args(sc, gpu)
    device, dev_index, P, g, st, held = _scene_structs(
        a["bg"], a["means3D"], a["colors"], a["opacities"], a["scales"], a["rotations"], a["mod"],
        a["cov6"], a["view"], a["proj"], a["tx"], a["ty"], sc["H"], sc["W"], a["sh"], a["deg"],
        a["campos"], False, False)
    y0, y1 = 0, sc["H"]
    if rows is not None:
        st.tile_row_begin, st.tile_row_end = rows
        y0, y1 = rows[0] * 16, min(sc["H"], rows[1] * 16)
    dL, dLp = ar.loss_gradients(sc, "combined" if planes else "colour")
    dL = to_dev(np.ascontiguousarray(dL[:, y0:y1]), gpu)
    f32 = dict(dtype=torch.float32, device=device)
    grads = {"dL_dmeans3D": (P, 3), "dL_dmeans2D": (P, 3), "dL_dopacity": (P, 1),
             "dL_dcolors": (P, 3), "dL_dcov3D": (P, 6)}
    if g.shs:
        grads["dL_dsh"] = (P, g.M, 3)
    if g.scales:
        grads.update(dL_dscales=(P, 3), dL_drotations=(P, 4))
    grads = {n: torch.zeros(shape, **f32) for n, shape in grads.items()}
    out = _lib.GsrGradients(**{n: t.data_ptr() for n, t in grads.items()})
    optional = [None] * 5
    if planes:
        dLp = [to_dev(np.ascontiguousarray(p[y0:y1]), gpu) for p in dLp]
        optional[0] = _lib.GsrPlaneGradients(dL_ddepth_map=dLp[0].data_ptr(),
                                             dL_dinv_depth_map=dLp[1].data_ptr(),
                                             dL_dfinal_T=dLp[2].data_ptr())
    cam = {}
    if camera:
        cam = {"dL_dviewmatrix": torch.zeros((4, 4), **f32),
               "dL_dprojmatrix": torch.zeros((4, 4), **f32), "dL_dcampos": torch.zeros((3,), **f32)}
        optional[1] = _lib.GsrCameraGradients(**{n: t.data_ptr() for n, t in cam.items()})
    if aa:
        optional[2] = _lib.GsrFilterSettings(antialiasing=1)
    if det:
        optional[3] = _lib.GsrBackwardOrder(deterministic=1)
    n = ENTRIES[entry]
    assert all(s is None for s in optional[n:]), f"{entry} cannot express the request"
    inp = _lib.GsrBackwardInputs(dL_dcolor=dL.data_ptr())
    lib = _lib.load_library()
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    with torch.cuda.device(dev_index):
        _lib.check(getattr(lib, entry)(
            _lib.context(dev_index), ctypes.byref(g), ctypes.byref(st), ctypes.byref(inp),
            *(None if s is None else ctypes.byref(s) for s in optional[:n]), ctypes.byref(out),
            stream), entry)
    grads.update(cam)
    if camera and sc["colors"] is not None:  # (no SH: nothing reads campos)
        grads.pop("dL_dcampos")
    return {k: v.cpu().numpy() for k, v in grads.items()}


def _f64(got):
    return {k: v.astype(np.float64) for k, v in got.items()}


OPTIONS = {"plain": {}, "planes": dict(planes=True), "camera": dict(planes=True, camera=True),
           "antialiasing": dict(aa=True)}


@pytest.mark.parametrize("option", sorted(OPTIONS))
@pytest.mark.parametrize("name", SCENES)
def test_deterministic_entries_give_the_same_bits(name, option, gpu):
    sc, kw = aa_scenes.get(name), OPTIONS[option]
    for rows, entries in ((None, ("gsr_backward_features", "gsr_backward_strip",
                                  "gsr_backward_ordered")),
                          (STRIP, ("gsr_backward_features", "gsr_backward_strip"))):
        want = _call(entries[0], sc, gpu, det=True, rows=rows, **kw)
        assert any(v.any() for v in want.values())
        for entry in entries[1:]:
            got = _call(entry, sc, gpu, det=True, rows=rows, **kw)
            assert set(got) == set(want)
            for k in want:
                np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]),
                                              err_msg=f"{name}/{option}/{rows}/{entry}: {k}")


@pytest.mark.parametrize("name", SCENES)
def test_atomic_entries_meet_their_references(name, gpu):
    sc = aa_scenes.get(name)
    top = "gsr_backward_features"
    for entry, mode, kw in (("gsr_backward", "colour", {}),
                            ("gsr_backward_planes", "planes", dict(planes=True)),
                            ("gsr_backward_camera", "camera", dict(planes=True, camera=True)),
                            ("gsr_backward_filtered", "camera", dict(planes=True, camera=True)),
                            (top, "colour", {}), (top, "camera", dict(planes=True, camera=True))):
        _assert_plain_close(_f64(_call(entry, sc, gpu, **kw)), sc, gpu, mode, f"{name}/{entry}")
    for entry in ("gsr_backward_filtered", top):
        got = _f64(_call(entry, sc, gpu, planes=True, camera=True, aa=True))
        _assert_close(got, _aa_reference(sc, gpu, "combined"), f"{name}/{entry}/antialiasing")
    # `_C`: upstream's entry (gsr_backward), and everything else through the top entry with NULLs
    _lib.context(gpu.index or 0)
    _assert_plain_close(_run(sc, gpu, "colour", False)[1], sc, gpu, "colour", f"{name}/_C upstream")
    _assert_plain_close(_run(sc, gpu, "camera", False)[1], sc, gpu, "camera", f"{name}/_C general")
    _assert_close(_run(sc, gpu, "camera", True)[1], _aa_reference(sc, gpu, "combined"),
                  f"{name}/_C general/antialiasing")
