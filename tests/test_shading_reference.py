"""The float64 reference of the GL shadings (shading_reference.py) on the CPU: the vectorised
form equals a per-pixel loop, every scene of shading_scenes.py keeps its unstable share under the
cap in every shading and reaches what it was built for, and the C ABI declares the entry point
the GPU tests (test_gpu_shading.py) render through."""
import os
import re

import numpy as np
import pytest

from gaussiansplattingviewer_amd import _lib

import shading_reference as sr
import shading_scenes as ss
from gpu_helpers import UNSTABLE_CAP

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "gsr.h")


@pytest.fixture(scope="module")
def scenes(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            sc = ss.build(oracle_mod, name)
            ss.run(oracle_mod, sc)
            cache[name] = sc
        return cache[name]
    return get


@pytest.mark.parametrize("name", ("sparse", "ragged_7x5"))
@pytest.mark.parametrize("shading", ss.SHADINGS)
def test_vectorised_reference_equals_pixel_loop(scenes, name, shading):
    sc = scenes(name)
    orc = sc["orc"]
    ref = sr.reference(sc, orc, shading)
    loop = sr.render_loop(orc["ranges"], orc["point_list"], orc["means2D"], orc["conic_opacity"],
                          ref["features"], sc["s"]["bg"], sc["W"], sc["H"], shading)
    for k in ("n_contrib", "final_T", "stable"):
        np.testing.assert_array_equal(ref[k], loop[k], err_msg=k)
    np.testing.assert_allclose(ref["color"].astype(np.float64), loop["color"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(ref["bound"], loop["bound"], rtol=1e-12, atol=0)
    assert (ref["n_contrib"] > 0).any()
    assert name != "sparse" or (ref["n_contrib"] == 0).any()


def _pixels(mask):
    return {(int(x), int(y)) for y, x in np.argwhere(mask)}


@pytest.mark.parametrize("name", ss.NAMES)
@pytest.mark.parametrize("shading", ss.SHADINGS)
def test_scene_is_stable_and_reaches_its_events(scenes, name, shading):
    sc = scenes(name)
    orc = sc["orc"]
    ref = sr.reference(sc, orc, shading)
    st, nc = ref["stable"], ref["n_contrib"]
    share = 1.0 - float(st.mean())
    print(f"{name} shading {shading}: unstable {share:.5f}, hits {float((nc > 0).mean()):.3f}")
    assert share <= UNSTABLE_CAP
    assert (nc <= ref["list_len"]).all()
    assert ((ref["final_T"] == 0.0) == (nc > 0)).all()
    ball = shading != sr.BILLBOARD
    if name.startswith("first_hit_"):
        n = int(name.rsplit("_", 1)[1])
        assert (ref["list_len"] == n).all() and st.all()
        assert (nc == (n if ball else 1)).all()
    elif name == "sparse":
        assert 0.1 <= float((nc > 0).mean()) <= 0.9
    elif name == "mixed":
        assert (nc > 1).mean() > 0.2  # hits behind entries that miss
    elif name == "threshold_edges":
        op = sc["s"]["g"].opacity.reshape(-1)
        np.testing.assert_array_equal(orc["means2D"], np.asarray(sc["targets"], np.float32))
        for v in ss.THRESHOLD_OPACITIES:
            assert (op.view(np.uint32) == v.view(np.uint32)).sum() == 2
        want = {(int(x), int(y)) for (x, y), o in zip(sc["targets"], op) if o > ss.O_MIN} \
            if ball else set()
        assert _pixels(~st) == want and (len(want) == 6 or not ball)
        if ball:  # only the centre pixel of an opacity above 0.22f is painted
            assert _pixels(nc > 0) == want
    elif name == "quad_edges":
        q = sc["quads"]
        on = q[:, 3] == 0.0
        np.testing.assert_array_equal(orc["means2D"][on], q[on, :2].astype(np.float32))
        yy, xx = np.mgrid[0:sc["H"], 0:sc["W"]]
        if ball:
            want = {(int(x), int(y)) for x, y in q[:, :2]}
        else:
            want = set()
            for x, y, e, _ in q[on]:
                want |= _pixels(np.maximum(np.abs(xx - x), np.abs(yy - y)) == e)
            # quads 1e-3 px beside a pixel: the edge column is inside on one side only
            for x, y, e, off in q[~on]:
                s = int(np.sign(off))
                assert nc[int(y), int(x) + s * int(e)] > 0 and nc[int(y), int(x) - s * int(e)] == 0
        assert len(want) > 0 and _pixels(~st) == want
    elif name == "front_transparent":
        if ball:
            assert (nc != 1).all() and (nc >= 2).sum() >= 20
        else:
            assert (nc == 1).all()
            assert (ref["color"] == np.asarray(sc["colors"][0], np.float32)[:, None, None]).all()


def test_mode3_bound_is_first_order_in_the_power_error(scenes):
    """The gaussian ball's bound: relative to the colour, expm1(dp) + 4 u, with dp under 1/4 on
    every stable pixel; shadings 1 and 2 carry no bound."""
    sc = scenes("mixed")
    ref = sr.reference(sc, sc["orc"], sr.GAUSS_BALL)
    hit = ref["stable"] & (ref["n_contrib"] > 0)
    cmax = np.abs(ref["color"]).max(axis=0)
    assert hit.sum() > 500
    rel = ref["bound"][hit] / cmax[hit]
    assert (rel >= 4.0 * sr.U).all() and rel.max() < 1e-3
    assert (ref["bound"][ref["n_contrib"] == 0] == 0).all()
    assert not sr.reference(sc, sc["orc"], sr.FLAT_BALL)["bound"].any()


def test_abi_declares_the_shaded_forward():
    """include/gsr.h and _lib agree on the GSR_SHADE_* values; gsr_forward_shaded is declared,
    listed and exported; the ABI is 4."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ids = {k: int(v) for k, v in re.findall(r"\b(GSR_SHADE_[A-Z_]+)\s*=\s*(\d+)", src)}
    assert ids == {"GSR_SHADE_SPLAT": 0, "GSR_SHADE_BILLBOARD": 1, "GSR_SHADE_FLAT_BALL": 2,
                   "GSR_SHADE_GAUSS_BALL": 3}
    assert ids == {k: getattr(_lib, k) for k in dir(_lib) if k.startswith("GSR_SHADE_")}
    assert re.search(r"\bint\s+gsr_forward_shaded\s*\(", src)
    assert "gsr_forward_shaded" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load_library()
    assert hasattr(lib, "gsr_forward_shaded")
    assert re.search(r"#define\s+GSR_ABI_VERSION\s+4\b", src)
    assert _lib.ABI_VERSION == 4 and lib.gsr_abi_version() == 4
    assert (ss.SHADINGS == (_lib.GSR_SHADE_BILLBOARD, _lib.GSR_SHADE_FLAT_BALL,
                            _lib.GSR_SHADE_GAUSS_BALL) == (sr.BILLBOARD, sr.FLAT_BALL,
                                                           sr.GAUSS_BALL))


def test_python_api_carries_the_shading():
    """GaussianRasterizationSettings ends in a defaulted `shading`; upstream's 12-field
    constructions are unaffected; HIPRenderer takes gl_shading."""
    import inspect

    from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                        rasterize_gaussians_native)
    from gaussiansplattingviewer_amd.renderer import HIPRenderer
    assert GaussianRasterizationSettings._fields[-1] == "shading"
    assert GaussianRasterizationSettings._field_defaults == {"shading": 0}
    rs = GaussianRasterizationSettings(4, 6, 0.5, 0.4, None, 1.0, None, None, 3, None, False, False)
    assert rs.shading == 0 and rs.debug is False
    p = inspect.signature(rasterize_gaussians_native).parameters["shading"]
    assert p.default == 0 and p.kind is inspect.Parameter.KEYWORD_ONLY
    params = list(inspect.signature(HIPRenderer.__init__).parameters.values())
    assert [q.name for q in params] == ["self", "w", "h", "device", "tile_rows", "gl_shading"]
    assert params[-1].default is False
    assert HIPRenderer.GL_SHADINGS == {-2: 1, -3: 2, -4: 3}
