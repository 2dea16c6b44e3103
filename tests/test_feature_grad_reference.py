"""CPU: pins the reference of the feature-channel tests (feature_grad_reference) against the oracle,
asserts the condition on the scenes (no decision within rounding of its gate under the features'
losses), re-measures the float32 spread the GPU tolerance is built from, and checks the host side of
gsr_forward_features / gsr_backward_features: exported, their structs laid out as the header's,
refusing bad arguments before any device call; GaussianRasterizer and ForwardResult keep their
shapes without features."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import feature_grad_reference as fg
import grad_reference as gr
import grad_scenes
import oracle
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd import rasterizer as rz
from test_grad_reference import _oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ref_cache = {}


def _ref64(sc, loss, C):
    """The float64 reference on the oracle's lists."""
    key = (sc["name"], loss, C)
    if key not in _ref_cache:
        orc = _oracle(sc)
        _ref_cache[key] = fg.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"],
                                             *fg.loss_gradients(sc, loss, C))
    return _ref_cache[key]


@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_feature_map_matches_render_f64(name):
    """feature_map_of on the oracle's float32 records is the oracle's float64 blend of the same
    features as colours with bg = 0, three channels at a time; the planes are not degenerate and
    carry both signs."""
    sc = grad_scenes.get(name)
    orc = _oracle(sc)
    C = 5
    feat = fg.feature_rows(name, C)
    t = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64))  # noqa: E731
    lists = (orc["ranges"], orc["point_list"])
    with torch.no_grad():
        _, gates, near = gr.composite(lists, t(orc["means2D"]), t(orc["conic_opacity"][:, :3]),
                                      t(orc["conic_opacity"][:, 3]), t(feat[:, :3]), fg.ZERO_BG,
                                      sc["W"], sc["H"])
        fmap = fg.feature_map_of(lists, t(orc["means2D"]), t(orc["conic_opacity"][:, :3]),
                                 t(orc["conic_opacity"][:, 3]), t(feat), sc["W"], sc["H"],
                                 gates).numpy()
    assert near == 0 and fmap.shape == (C, sc["H"], sc["W"])
    for j in (0, 3):
        cols = np.zeros((len(feat), 3), np.float32)
        cols[:, :min(3, C - j)] = feat[:, j:j + 3]
        f64 = oracle.render_f64(orc["ranges"], orc["point_list"], orc["means2D"],
                                orc["conic_opacity"], cols, (0.0, 0.0, 0.0), sc["W"], sc["H"])
        assert np.abs(fmap[j:j + 3] - f64["color"][:min(3, C - j)]).max() <= 1e-12
    assert fmap.max() > 0.1 and fmap.min() < -0.1


@pytest.mark.parametrize("C", fg.CHANNELS)
@pytest.mark.parametrize("loss", fg.LOSSES)
@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_no_decision_near_its_gate(name, loss, C):
    ref = _ref64(grad_scenes.get(name), loss, C)
    assert ref["near"] == (0, 0, 0)
    assert ref["features"].shape[1] == C and np.abs(ref["features"]).max() > 0
    assert (ref["rgb"] == 0).all() == (loss == "features")


def test_culled_rows_get_zero_feature_gradients():
    """S4: the reference gives exact zeros to the features of Gaussians with radii == 0."""
    sc = grad_scenes.get("edges")
    orc, ref = _oracle(sc), _ref64(grad_scenes.get("edges"), "features", 5)
    assert (orc["radii"] == 0).any() and (ref["features"][orc["radii"] == 0] == 0).all()


def test_float32_spread_constants():
    """fg.F32_SPREAD (the GPU tests' yardstick) is what a float32 evaluation of the reference gives
    here under the losses and channel counts the GPU tests feed, to within a factor 2 either
    way."""
    seen = {}
    for name in grad_scenes.NAMES:
        sc = grad_scenes.get(name)
        orc = _oracle(sc)
        for loss in fg.LOSSES:
            for C in fg.CHANNELS:
                r64 = _ref64(sc, loss, C)
                r32 = fg.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"],
                                         *fg.loss_gradients(sc, loss, C), None, torch.float32,
                                         r64["gates"])
                for k in fg.F32_SPREAD:
                    if k in r64 and np.abs(r64[k]).max() > 0:
                        seen[k] = max(seen.get(k, 0.0), gr.rel_err(r32[k], r64[k]))
    print({k: f"{v:.3e}" for k, v in seen.items()})
    assert set(seen) == set(fg.F32_SPREAD)
    for k, f in seen.items():
        assert 0.5 * f <= fg.F32_SPREAD[k] <= 2.0 * f, (k, f, fg.F32_SPREAD[k])


def test_float32_spread_constants_everything_at_once():
    """fg.F32_SPREAD_ALL, the same way, for colour, planes, features, the antialiased forward and
    the camera's gradients together on S1; no decision near its gate there either."""
    sc = grad_scenes.get(fg.ALL_SCENE)
    orc = _oracle(sc)
    lists = (orc["ranges"], orc["point_list"])
    r64 = fg.all_gradients(sc, lists, orc["radii"])
    r32 = fg.all_gradients(sc, lists, orc["radii"], torch.float32, r64["gates"])
    assert r64["near"] == (0, 0, 0)
    for k, c in fg.F32_SPREAD_ALL.items():
        f = fg.err(r32[k], r64, k)
        print(f"{k}: {f:.3e}")
        assert np.isfinite(r64[k]).all() and 0.5 * f <= c <= 2.0 * f, (k, f, c)


def test_features_are_linear_in_the_channel_set():
    """The derivation the kernels' split into passes rests on: the geometry's
    gradients under colour plus features are the sum of those under each alone, and dL_dfeatures
    does not depend on the colour's gradient."""
    sc = grad_scenes.get("chain")
    orc = _oracle(sc)
    both, feat = _ref64(sc, "combined", 5), _ref64(sc, "features", 5)
    colour = gr.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"], sc["dL"])
    for k in ("means2D_px", "conic", "opacity", "means3D"):
        assert gr.rel_err(feat[k] + colour[k], both[k]) <= 1e-12, k
    assert gr.rel_err(feat["features"], both["features"]) <= 1e-14
    assert gr.rel_err(colour["rgb"], both["rgb"]) <= 1e-14


def _probe(tmp_path, struct, names):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsr.h"', "int main(void){",
             f'printf("size %zu\\n", sizeof({struct}));',
             'printf("max %d\\n", GSR_MAX_FEATURES);']
    lines += [f'printf("{f} %zu\\n", offsetof({struct}, {f}));' for f in names]
    lines += ["return 0;}"]
    src = tmp_path / f"{struct}.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / struct
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    return {ln.split()[0]: int(ln.split()[1]) for ln in out if ln}


def test_features_host_abi(tmp_path):
    """The two entries are exported and refuse bad arguments before any device call; the ctypes
    structs are laid out as the header's; the ABI version stays 4."""
    lib = _lib.load_library()
    for name in ("gsr_forward_features", "gsr_backward_features"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.gsr_abi_version() == _lib.ABI_VERSION == 4
    for struct, cls in (("gsr_feature_outputs", _lib.GsrFeatureOutputs),
                        ("gsr_feature_gradients", _lib.GsrFeatureGradients)):
        names = [f for f, _ in cls._fields_]
        got = _probe(tmp_path, struct, names)
        assert got["size"] == ctypes.sizeof(cls) and got["max"] == _lib.MAX_FEATURES == 256
        for f in names:
            assert got[f] == getattr(cls, f).offset, (struct, f)

    fwd, bwd = _lib.features_fns(lib)
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)  # never dereferenced
    g, st = _lib.GsrGaussians(P=4), _lib.GsrRasterSettings(image_width=8, image_height=8)
    out, ref = _lib.GsrOutputs(), ctypes.byref
    for C, features, why in ((0, 64, b"C must be in 1..GSR_MAX_FEATURES"),
                             (257, 64, b"C must be in 1..GSR_MAX_FEATURES"),
                             (-1, 64, b"C must be in 1..GSR_MAX_FEATURES"),
                             (4, None, b"features is NULL")):
        fo = _lib.GsrFeatureOutputs(C=C, features=features, feature_map=64)
        assert fwd(ctx, ref(g), ref(st), ref(out), None, None, None, ref(fo), None) == -1
        assert b"gsr_forward_features" in lib.gsr_last_error() and why in lib.gsr_last_error()
        fgr = _lib.GsrFeatureGradients(C=C, features=features, dL_dfeature_map=64, dL_dfeatures=64)
        assert bwd(ctx, ref(g), ref(st), ref(_lib.GsrBackwardInputs()), None, None, None, None,
                   ref(fgr), ref(_lib.GsrGradients()), None) == -1
        assert b"gsr_backward_features" in lib.gsr_last_error() and why in lib.gsr_last_error()
    # the deterministic mode has no room for the features' sums, and says so
    fgr = _lib.GsrFeatureGradients(C=4, features=64, dL_dfeature_map=64, dL_dfeatures=64)
    order = _lib.GsrBackwardOrder(deterministic=1)
    assert bwd(ctx, ref(g), ref(st), ref(_lib.GsrBackwardInputs()), None, None, None, ref(order),
               ref(fgr), ref(_lib.GsrGradients()), None) == -1
    assert b"deterministic" in lib.gsr_last_error() and b"no room" in lib.gsr_last_error()
    # a feature gradient stands in for dL_dcolor: the next check is reached
    order.deterministic = 0
    assert bwd(ctx, ref(g), ref(st), ref(_lib.GsrBackwardInputs()), None, None, None, ref(order),
               ref(fgr), ref(_lib.GsrGradients()), None) == -1
    assert b"SHs or precomputed colors" in lib.gsr_last_error()
    # without a map the entries are the ones they extend: their messages
    fgr.dL_dfeature_map = None
    assert bwd(ctx, ref(g), ref(st), ref(_lib.GsrBackwardInputs()), None, None, None, None,
               ref(fgr), ref(_lib.GsrGradients()), None) == -1
    assert b"dL_dcolor is required" in lib.gsr_last_error()


def test_python_signatures_are_additive():
    """features is the last parameter of GaussianRasterizer.forward and keyword-only in the native
    wrappers, None by default; ForwardResult gains a trailing feature_map that defaults to None;
    strips.reduce_gradients' docstring names dL_dfeatures."""
    from gaussiansplattingviewer_amd import strips
    params = list(inspect.signature(rz.GaussianRasterizer.forward).parameters.values())
    assert params[-1].name == "features" and params[-1].default is None
    assert [p.name for p in params[1:9]] == ["means3D", "means2D", "opacities", "shs",
                                             "colors_precomp", "scales", "rotations",
                                             "cov3D_precomp"]
    for fn, names in ((rz.rasterize_gaussians_native, ("features",)),
                      (rz.rasterize_gaussians_backward_native, ("features", "dL_dfeature_map"))):
        sig = inspect.signature(fn).parameters
        for n in names:
            assert sig[n].kind is inspect.Parameter.KEYWORD_ONLY and sig[n].default is None
    assert rz.ForwardResult._fields == ("num_rendered", "color", "radii", "extras", "feature_map")
    assert rz.ForwardResult(1, None, None, {}).feature_map is None
    assert "dL_dfeatures" in strips.reduce_gradients.__doc__
    with pytest.raises(RuntimeError, match="num_points, C"):
        rz._feature_rows(torch.zeros(3, 2, 2), 3, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="outside 1..256"):
        rz._feature_rows(torch.zeros(3, 257), 3, torch.device("cpu"))
