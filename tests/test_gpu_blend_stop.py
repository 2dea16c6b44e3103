"""The early exit of the blend's composite loop (csrc/blend.hip kStopPairs) on the device, on the
scenes of stop_scenes.py (test_stop_scenes.py asserts on the CPU that each terminates where it
says): every scene in both arithmetic modes per pixel against the float64 reference, the quadrant
cull on and off and the viewer's plain call (the paired-slot kernel) bit-identical; a stop_S scene
without the splats behind position S renders the same bits (what the exit skips adds nothing);
and one stop_S and stop_spread through gsr_forward_depth and gsr_forward_surface against the
references of those suites (depth_scenes, median_reference)."""
import numpy as np
import pytest

from gaussiansplattingviewer_amd import _lib

import blend_scenes as bs
import depth_scenes as ds
import median_reference as mr
import stop_scenes as ss
from gpu_helpers import ALL_EXTRAS, assert_blend_exact, run_hip, set_option

pytestmark = pytest.mark.gpu

PIXELS = ("color", "final_T", "n_contrib")
SURF = ("median_depth", "median_id")


def _render(sc, gpu, **kw):
    return run_hip(sc["s"], gpu, colors_precomp=sc["colors"], cov3D_precomp=sc["cov6"], **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


@pytest.fixture(scope="module")
def scenes(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            sc = ss.build(oracle_mod, name)
            bs.run(oracle_mod, sc)
            cache[name] = sc
        return cache[name]
    return get


@pytest.fixture
def options(gpu):
    """The context's blend options, restored to their defaults afterwards."""
    try:
        yield lambda opt, v: set_option(gpu, opt, v)
    finally:
        set_option(gpu, _lib.GSR_OPT_BLEND_FAST, 1)
        set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 1)


@pytest.mark.parametrize("name", ss.NAMES)
def test_blend_exact_on_stop_scene(gpu, oracle_mod, scenes, options, name):
    sc = scenes(name)
    orc = sc["orc"]
    bg, feats = sc["s"]["bg"], bs.features(sc, orc)
    cut = scenes(name + "_cut") if name[5:].isdigit() else None
    for fast in (1, 0):
        what = f"{name} {'fast' if fast else 'exact'}"
        options(_lib.GSR_OPT_BLEND_FAST, fast)
        options(_lib.GSR_OPT_BLEND_CULL, 0)
        off = _render(sc, gpu)
        options(_lib.GSR_OPT_BLEND_CULL, 1)
        hip = _render(sc, gpu)
        assert_blend_exact(oracle_mod, off, orc, bg, feats, what=what + " no cull")
        assert_blend_exact(oracle_mod, hip, orc, bg, feats, what=what)
        for k in PIXELS:
            np.testing.assert_array_equal(_bits(hip[k]), _bits(off[k]),
                                          err_msg=f"{what}: cull changes {k}")
        plain = _render(sc, gpu, extras=(), binning=False)
        np.testing.assert_array_equal(_bits(plain["color"]), _bits(hip["color"]),
                                      err_msg=f"{what}: plain call")
        if cut is not None:
            # truncation identity: the list's head alone, with n_contrib and without
            head = _render(cut, gpu, binning=False)
            for k in PIXELS:
                np.testing.assert_array_equal(_bits(head[k]), _bits(hip[k]),
                                              err_msg=f"{what}: splats behind S change {k}")
            head = _render(cut, gpu, extras=(), binning=False)
            np.testing.assert_array_equal(_bits(head["color"]), _bits(plain["color"]),
                                          err_msg=f"{what}: splats behind S, plain call")


@pytest.mark.parametrize("name", ("stop_66", "stop_spread"))
def test_depth_and_median_planes_on_stop_scene(gpu, oracle_mod, scenes, options, name):
    sc = scenes(name)
    orc = sc["orc"]
    dref = ds.reference(oracle_mod, sc, orc)
    mref = mr.reference(oracle_mod, sc, orc)
    mr.assert_scene_decides(mref, name)
    for fast in (1, 0):
        what = f"{name} {'fast' if fast else 'exact'}"
        options(_lib.GSR_OPT_BLEND_FAST, fast)
        plain = _render(sc, gpu, binning=False)
        # gsr_forward_depth, with n_contrib and (the paired-slot form) without
        dep = _render(sc, gpu, extras=ALL_EXTRAS + ds.PLANES, binning=False)
        few = _render(sc, gpu, extras=ds.PLANES, binning=False)
        for k in ds.PLANES:
            ds.assert_plane_exact(dep[k], dep["n_contrib"], dref[k], f"{what} {k}")
            np.testing.assert_array_equal(_bits(few[k]), _bits(dep[k]), err_msg=f"{what}: {k} alone")
        for k in PIXELS:
            np.testing.assert_array_equal(_bits(dep[k]), _bits(plain[k]), err_msg=f"{what}: {k}")
        # gsr_forward_surface: without and with the depth planes, with n_contrib and without
        for extras in (ALL_EXTRAS + SURF, ALL_EXTRAS + ds.PLANES + SURF, SURF, ds.PLANES + SURF):
            sur = _render(sc, gpu, extras=extras, binning=False)
            mr.assert_median_accepted(mref, sc, sur["median_id"], sur["median_depth"],
                                      dep["depths"], f"{what} {len(extras)} extras")
            for k in ("color",) + tuple(k for k in PIXELS[1:] + ds.PLANES if k in extras):
                np.testing.assert_array_equal(_bits(sur[k]), _bits(dep[k]),
                                              err_msg=f"{what}: surface call, {k}")
