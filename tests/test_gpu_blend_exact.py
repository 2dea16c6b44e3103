"""The blend kernel per pixel against the float64 reference (gpu_helpers.assert_blend_exact) on
the edge scenes of blend_scenes.py: every scene in both arithmetic modes, with the quadrant cull
on and off (bit-identical to each other), through the viewer's plain call (no extras: the
paired-slot kernel, tight lists; bit-identical colour) and, where the frame has two tile rows,
as two strips whose rows equal the full frame's.  test_blend_reference.py asserts on the CPU that
each scene reaches the paths it was built for and that the oracle alone meets the same
assertions."""
import numpy as np
import pytest

from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.strips import strip_pixel_rows

import blend_scenes as bs
from gpu_helpers import assert_blend_exact, run_hip, set_option

pytestmark = pytest.mark.gpu


def _render(sc, gpu, **kw):
    return run_hip(sc["s"], gpu, colors_precomp=sc["colors"], cov3D_precomp=sc["cov6"], **kw)


@pytest.mark.parametrize("name", bs.NAMES)
def test_blend_exact_on_edge_scene(gpu, oracle_mod, name):
    sc = bs.build(oracle_mod, name)
    orc = bs.run(oracle_mod, sc)
    bg, feats = sc["s"]["bg"], bs.features(sc, orc)
    gy = (sc["H"] + 15) // 16
    try:
        for fast in (1, 0):
            set_option(gpu, _lib.GSR_OPT_BLEND_FAST, fast)
            set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 0)
            off = _render(sc, gpu)
            set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 1)
            hip = _render(sc, gpu)
            what = f"{name} {'fast' if fast else 'exact'}"
            assert_blend_exact(oracle_mod, off, orc, bg, feats, what=what + " no cull")
            assert_blend_exact(oracle_mod, hip, orc, bg, feats, what=what)
            for k in ("color", "final_T", "n_contrib"):
                np.testing.assert_array_equal(hip[k].view(np.uint32), off[k].view(np.uint32),
                                              err_msg=f"{what}: cull changes {k}")
            plain = _render(sc, gpu, extras=(), binning=False)
            np.testing.assert_array_equal(plain["color"].view(np.uint32),
                                          hip["color"].view(np.uint32),
                                          err_msg=f"{what}: plain call")
            if gy >= 2:
                for rows in ((0, 1), (1, gy)):
                    part = _render(sc, gpu, tile_rows=rows, binning=False)
                    y0, n = strip_pixel_rows(rows, sc["H"])
                    for k in ("color", "final_T", "n_contrib"):
                        np.testing.assert_array_equal(
                            part[k].view(np.uint32), hip[k][..., y0:y0 + n, :].view(np.uint32),
                            err_msg=f"{what}: strip {rows} {k}")
    finally:
        set_option(gpu, _lib.GSR_OPT_BLEND_FAST, 1)
        set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 1)
