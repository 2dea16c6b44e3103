"""The per-Gaussian stage (csrc/preprocess.hip) on the edge scenes of preprocess_scenes.py, on
the GPU: parity with the oracle (floats bit-equal or both NaN), the image independent of which
extras the caller asked for, lean strips (k_preprocess<true>, strip_reach) equal to the full
frame's rows, inputs that are not 16-byte aligned (the scalar-load branches), frame graphs and
the depth-sort forms.  test_preprocess_reference.py shows on the CPU that each scene reaches the
edge it was built for and that the oracle is right on it.

`nonfinite*` and `scale_range_*` assert defined behaviour on hostile input: every integer the
kernels derive from a float is clamped before it indexes memory (f2i_sat saturates and maps NaN
to 0; getRect clamps each word to the grid; a span word's rows are clamped to the strip rect; a
non-positive radius is culled), so they render, with finite pixels, what the oracle renders."""
import numpy as np
import pytest

from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.camera import static_camera
from gaussiansplattingviewer_amd.gaussian_data import synthetic_gaussians
from gaussiansplattingviewer_amd.strips import strip_pixel_rows

import preprocess_scenes as ps
from gpu_helpers import (ALL_EXTRAS, assert_blend_exact, assert_image_close, run_hip, scene_inputs,
                         set_option, tight_binning)

pytestmark = pytest.mark.gpu

F32 = np.float32
FLOATS = ("depths", "means2D", "conic_opacity", "rgb")
PIXELS = ("color", "final_T", "n_contrib")


def _render(sc, gpu, **kw):
    return run_hip(sc["s"], gpu, colors_precomp=sc["colors"], cov3D_precomp=sc["cov6"], **kw)


def assert_parity_or_nan(hip, orc, image=True):
    """gpu_helpers.assert_parity with the preprocess floats held to assert_bits_or_nan: integer
    outputs, lists and ranges equal; floats bit-equal or both NaN; the image within tolerance."""
    assert hip["num_rendered"] == orc["num_rendered"]
    np.testing.assert_array_equal(hip["radii"], orc["radii"])
    np.testing.assert_array_equal(hip["tiles_touched"], orc["tiles_touched"])
    for k in FLOATS:
        ps.assert_bits_or_nan(hip[k], orc[k], k)
    np.testing.assert_array_equal(hip["point_list"], orc["point_list"])
    np.testing.assert_array_equal(hip["point_tiles"],
                                  (orc["point_keys"] >> np.uint64(32)).astype(np.uint32))
    np.testing.assert_array_equal(hip["ranges"], orc["ranges"])
    if image:
        assert_image_close(hip["color"], orc["color"])
        assert_image_close(hip["final_T"], orc["final_T"], "final_T")
        mism = float((hip["n_contrib"] != orc["n_contrib"]).mean())
        assert mism <= 1e-4, f"n_contrib differs at {mism:.2e} of pixels"


def _same_bits(a, b, what):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32),
                                  np.ascontiguousarray(b).view(np.uint32), err_msg=what)


@pytest.mark.parametrize("name", ps.NAMES)
def test_parity_on_edge_scene(gpu, oracle_mod, name):
    sc = ps.get(oracle_mod, name)
    orc = ps.run(oracle_mod, sc)
    hip = _render(sc, gpu)
    assert_parity_or_nan(hip, orc, image=False)


@pytest.mark.parametrize("name", ps.NAMES)
def test_image_on_edge_scene(gpu, oracle_mod, name):
    """The image of the same call, held to assert_image_close and, where the records are finite
    and the pixels decidable, to the float64 blend reference.

    `nonfinite` holds a Gaussian of opacity -inf: upstream's alpha = o exp(power) is -inf
    (skipped) where exp(power) > 0 and NaN, so min(0.99, NaN) = 0.99, where exp underflows to 0
    -- 19 pixels in the far corners of its two tiles, which the oracle paints.  Both arithmetic
    modes must paint them, with the quadrant cull on and off (the cull once dropped the splat
    there, and the fast mode's log2(-inf) = NaN painted its whole rect)."""
    sc = ps.get(oracle_mod, name)
    orc = ps.run(oracle_mod, sc)
    hip = _render(sc, gpu)
    assert np.isfinite(hip["color"]).all() and np.isfinite(hip["final_T"]).all()
    assert_parity_or_nan(hip, orc, image=True)
    if name not in ps.BLEND_NOT_EXACT:
        assert_blend_exact(oracle_mod, hip, orc, sc["s"]["bg"], ps.features(sc, orc),
                           parity=False, what=name)
    if name == "nonfinite":
        try:
            for fast, cull in ((1, 0), (0, 1), (0, 0)):
                set_option(gpu, _lib.GSR_OPT_BLEND_FAST, fast)
                set_option(gpu, _lib.GSR_OPT_BLEND_CULL, cull)
                assert_parity_or_nan(_render(sc, gpu), orc, image=True)
        finally:
            set_option(gpu, _lib.GSR_OPT_BLEND_FAST, 1)
            set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 1)


_decoy = {}


def _render_decoy(gpu):
    """A frame of 600 ordinary Gaussians, all in front of the camera, with colours no scene
    uses: it leaves its colours in every record of the context's workspace, so a record colour
    that the next frame fails to write cannot match by luck."""
    if not _decoy:
        g = synthetic_gaussians(600, 3, 77)
        g.xyz = (g.xyz * F32([0.5, 0.35, 0.5])).astype(F32)  # inside the frustum at every depth
        _decoy.update(s=scene_inputs(g, static_camera(160, 120), 3),
                      colors=np.full((600, 3), 7.0, F32))
    out = run_hip(_decoy["s"], gpu, colors_precomp=_decoy["colors"], extras=(), binning=False)
    assert (out["radii"] > 0).all()


@pytest.mark.parametrize("name", ps.NAMES)
def test_extras_do_not_change_the_image(gpu, oracle_mod, name):
    """color with no extras (tight lists, the strip-rect colour predicate), with all extras
    (full lists, the rgb predicate) and with full lists and no extras: bit-equal, each after a
    frame that left other colours in the workspace."""
    sc = ps.get(oracle_mod, name)
    _render_decoy(gpu)
    full = _render(sc, gpu, extras=ALL_EXTRAS, binning=False)
    _render_decoy(gpu)
    plain = _render(sc, gpu, extras=(), binning=False)
    _same_bits(plain["color"], full["color"], f"{name}: no extras vs all extras")
    _render_decoy(gpu)
    with tight_binning(gpu, 0):
        loose = _render(sc, gpu, extras=(), binning=False)
    _same_bits(loose["color"], full["color"], f"{name}: full lists, no extras vs all extras")


@pytest.mark.parametrize("name", ps.NAMES)
def test_lean_strips_equal_the_full_frame(gpu, oracle_mod, name):
    """radii=False selects k_preprocess<true>: a Gaussian is dropped on strip_reach's bound
    alone, so the bound must hold at the near plane, under the clamp and over the scale range."""
    sc = ps.get(oracle_mod, name)
    full = _render(sc, gpu, binning=False)
    gy = (sc["H"] + 15) // 16
    for n in sorted({min(2, gy), gy}):
        cuts = [round(i * gy / n) for i in range(n + 1)]
        for rows in zip(cuts[:-1], cuts[1:]):
            part = _render(sc, gpu, tile_rows=rows, extras=("final_T", "n_contrib"), radii=False,
                           binning=False)
            y0, h = strip_pixel_rows(rows, sc["H"])
            for k in PIXELS:
                _same_bits(part[k], full[k][..., y0:y0 + h, :], f"{name}: strip {rows} {k}")


UNALIGNED = (("sh_edges_3_16",) + tuple(f"boundaries_{p}" for p in ps.BOUNDARY_PS) +
             tuple(f"scale_range_{k}" for k in ps.SCALE_MODS))


@pytest.mark.parametrize("name", UNALIGNED)
def test_unaligned_inputs_equal_aligned(gpu, oracle_mod, name):
    """shs, rotations and means3D one float into a larger buffer: sh_vec4 = rot_vec4 = 0, the
    scalar-load branches of color_from_sh (degree 3) and front_one."""
    sc = ps.get(oracle_mod, name)
    a = _render(sc, gpu)
    u = _render(sc, gpu, unaligned=True)
    assert a.keys() == u.keys()
    for k in a:
        if k == "num_rendered":
            assert a[k] == u[k]
        elif k in FLOATS:
            ps.assert_bits_or_nan(u[k], a[k], f"{name}: {k}")
        else:
            _same_bits(u[k], a[k], f"{name}: {k}")


GRAPH_SCENES = ("nonfinite", "nonfinite_precomp") + tuple(f"boundaries_{p}" for p in ps.BOUNDARY_PS)
SLOT_DIRECT, SLOT_GRAPH = 92, 90


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", GRAPH_SCENES)
def test_frame_graphs_equal_direct(gpu, oracle_mod, name, mode):
    """GSR_OPT_FRAME_GRAPHS 1 (recorded graphs) and 2 (deferred-K chains) count K after the
    frame is queued: the image and num_rendered equal mode 0's, frame after frame."""
    sc = ps.get(oracle_mod, name)
    slot = SLOT_GRAPH + mode - 1
    set_option(gpu, _lib.GSR_OPT_FRAME_GRAPHS, 0, SLOT_DIRECT)
    set_option(gpu, _lib.GSR_OPT_FRAME_GRAPHS, mode, slot)
    want = _render(sc, gpu, extras=(), binning=False, slot=SLOT_DIRECT)
    for frame in range(3):
        got = _render(sc, gpu, extras=(), binning=False, slot=slot)
        assert got["num_rendered"] == want["num_rendered"], (name, mode, frame)
        _same_bits(got["color"], want["color"], f"{name}: mode {mode} frame {frame}")
        np.testing.assert_array_equal(got["radii"], want["radii"])


@pytest.mark.parametrize("form", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["near_plane", "nonfinite"])
def test_depth_sort_forms_keep_the_list(gpu, oracle_mod, name, form):
    """Every depth-sort form (LSD, compacting, MSD, compacting MSD) on keys next to the near
    plane's 0x3E4CCCCD among culled 0xFFFFFFFF ones: the oracle's point list."""
    sc = ps.get(oracle_mod, name)
    orc = ps.run(oracle_mod, sc)
    set_option(gpu, _lib.GSR_OPT_DEPTH_SORT, form)
    try:
        hip = _render(sc, gpu)
    finally:
        set_option(gpu, _lib.GSR_OPT_DEPTH_SORT, -1)
    np.testing.assert_array_equal(hip["point_list"], orc["point_list"])
    np.testing.assert_array_equal(hip["ranges"], orc["ranges"])
    _same_bits(hip["depths"], orc["depths"], "depths")
    if name == "near_plane":
        kept = orc["depths"][orc["radii"] > 0].view(np.uint32)
        assert kept.min() == F32(0.2).view(np.uint32) + 1 == 0x3E4CCCCE
