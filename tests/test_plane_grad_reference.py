"""CPU: pins the reference of the plane-gradient tests (plane_grad_reference) against the oracle,
checks it with torch.autograd.gradcheck, asserts the condition on the scenes (no decision within
rounding of its gate), re-measures the float32 spread the GPU tolerance is built from, and checks
the host side of gsr_backward_planes: exported, its struct laid out as the header's, validating
without a device; GaussianRasterizationSettings.depth_maps last and off by default."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import grad_reference as gr
import grad_scenes
import oracle
import plane_grad_reference as pg
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import GaussianRasterizationSettings
from test_grad_reference import _oracle, _tiny

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ref_cache = {}


def _ref64(sc, loss):
    """The float64 reference on the oracle's lists; loss: a name pg.loss_gradients knows."""
    key = (sc["name"], loss)
    if key not in _ref_cache:
        orc = _oracle(sc)
        _ref_cache[key] = pg.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"],
                                             *pg.loss_gradients(sc, loss))
    return _ref_cache[key]


@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_planes_match_render_f64(name):
    """The three channels of composite(feat = (z, 1 / z, 0), bg = (0, 0, 1)) on the oracle's float32
    records are the oracle's float64 blend of the same features with bg = 0, and its final_T; the
    restated z is the oracle's `depths` to float32 rounding; the planes are not degenerate."""
    sc = grad_scenes.get(name)
    orc = _oracle(sc)
    z32 = np.where(orc["radii"] > 0, orc["depths"], 1.0).astype(np.float32)
    feat = np.stack([z32, np.float32(1.0) / z32, np.zeros_like(z32)], 1).astype(np.float32)
    feat[orc["radii"] == 0] = 0
    f64 = oracle.render_f64(orc["ranges"], orc["point_list"], orc["means2D"], orc["conic_opacity"],
                            feat, (0.0, 0.0, 0.0), sc["W"], sc["H"])
    t = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64))  # noqa: E731
    with torch.no_grad():
        planes, _, near = pg.planes_of((orc["ranges"], orc["point_list"]), t(orc["means2D"]),
                                       t(orc["conic_opacity"][:, :3]), t(orc["conic_opacity"][:, 3]),
                                       t(feat), sc["W"], sc["H"])
    assert near == 0
    planes = planes.numpy()
    assert np.abs(planes[:2] - f64["color"][:2]).max() <= 1e-12
    assert np.abs(planes[2] - f64["final_T"]).max() <= 1e-12
    assert planes[0].max() > 1.0 and planes[1].max() > 0.1 and 0.2 <= planes[2].max() <= 1.0
    # z: six float32 roundings (three products, three sums), each within 2^-24 of the terms' size
    xyz = torch.tensor(sc["s"]["g"].xyz.astype(np.float64))
    cam = gr.camera_constants(sc["s"])
    z = pg.view_depth(cam, orc["radii"], xyz).numpy()
    vm = cam["view"]
    size = (np.abs(xyz.numpy()) * np.abs([vm[2], vm[6], vm[10]])).sum(1) + abs(vm[14])
    vis = orc["radii"] > 0
    assert (np.abs(z - orc["depths"])[vis] <= 6 * 2.0 ** -24 * size[vis]).all()
    assert (z[~vis] == 0).all()
    # ... and features(z) of the reference: (z, 1 / z, 0), zero rows for the culled
    f = pg.features(torch.tensor(z), orc["radii"]).numpy()
    assert np.abs(f[vis, 1] * z[vis] - 1).max() <= 1e-15 and (f[~vis] == 0).all()
    assert (f[:, 2] == 0).all()


def test_gradcheck_planes():
    """gradcheck of the plane loss's two stages on the 8 x 8 scene of test_grad_reference."""
    sc = _tiny()
    orc = _oracle(sc)
    assert (orc["radii"] > 0).all()
    lists = (orc["ranges"], orc["point_list"])
    cam = gr.camera_constants(sc["s"])
    lv = gr.leaves(sc, torch.float64)
    assert torch.autograd.gradcheck(lambda x: pg.view_depth(cam, orc["radii"], x), (lv["means3D"],),
                                    eps=1e-6, atol=1e-7)
    with torch.no_grad():
        m2, conic, _, _, near_p = gr.project(cam, orc["radii"], lv["means3D"], lv["means2D"],
                                             lv["scales"], lv["rotations"], None, lv["shs"])
        z = pg.view_depth(cam, orc["radii"], lv["means3D"])
    leaves = [v.clone().requires_grad_(True) for v in (m2, conic, lv["opacity"].detach(), z)]
    _, gates_c, near_c = pg.planes_of(lists, *leaves[:3], pg.features(leaves[3], orc["radii"]), 8, 8)
    assert (near_p, near_c) == (0, 0)

    def planes(m2, conic, op, z):
        return pg.planes_of(lists, m2, conic, op, pg.features(z, orc["radii"]), 8, 8, gates_c)[0]
    assert torch.autograd.gradcheck(planes, tuple(leaves), eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("loss", pg.LOSSES)
@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_no_decision_near_its_gate(name, loss):
    ref = _ref64(grad_scenes.get(name), loss)
    assert ref["near"] == (0, 0)
    assert np.abs(ref["depths"]).max() > 0 and (ref["rgb"] == 0).all() == (loss == "planes")


def test_float32_spread_constants():
    """pg.F32_SPREAD (the GPU tests' yardstick) is what a float32 evaluation of the reference gives
    here under the losses the GPU tests feed, to within a factor 2 either way."""
    seen = {}
    for name in grad_scenes.NAMES:
        sc = grad_scenes.get(name)
        orc = _oracle(sc)
        for loss in pg.LOSSES + (pg.PLANES if name == pg.ONE_PLANE_SCENE else ()):
            r64 = _ref64(sc, loss)
            r32 = pg.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"],
                                     *pg.loss_gradients(sc, loss), torch.float32, r64["gates"])
            for k in pg.F32_SPREAD:
                if k in r64 and np.abs(r64[k]).max() > 0:
                    seen[k] = max(seen.get(k, 0.0), gr.rel_err(r32[k], r64[k]))
    print({k: f"{v:.3e}" for k, v in seen.items()})
    assert set(seen) == set(pg.F32_SPREAD)
    for k, f in seen.items():
        assert 0.5 * f <= pg.F32_SPREAD[k] <= 2.0 * f, (k, f, pg.F32_SPREAD[k])


def test_float32_spread_constants_disparity():
    """pg.F32_SPREAD_DISPARITY, the same way, for the metric_disparity loss on S1; the scene has
    no uncovered pixel, and dL is zero nowhere (no covered share below 1e-3)."""
    sc = grad_scenes.get("chain")
    orc = _oracle(sc)
    lists = (orc["ranges"], orc["point_list"])
    final_T = _ref64(sc, "planes")["planes"][2]
    assert final_T.max() < 0.95
    fn = pg.disparity_loss(sc, pg.disparity_dL("chain", final_T))
    r64 = pg.scene_gradients(sc, lists, orc["radii"], None, None, loss_fn=fn)
    r32 = pg.scene_gradients(sc, lists, orc["radii"], None, None, torch.float32, r64["gates"],
                             loss_fn=fn)
    assert r64["near"] == (0, 0) and (r64["shs"] == 0).all()
    for k, c in pg.F32_SPREAD_DISPARITY.items():
        f = gr.rel_err(r32[k], r64[k])
        print(f"{k}: {f:.3e}")
        assert np.isfinite(r64[k]).all() and 0.5 * f <= c <= 2.0 * f, (k, f, c)


def test_sign_of_the_inverse_depth_term_is_an_order_one_error():
    """The sensitivity of the dL_ddepths check, from the reference alone: with d(1 / z)/dz taken as
    +(1 / z)^2 the tenth sum is off by 0.19 of its size under the three-plane loss (10^4 bounds;
    gi / z^2 is about a tenth of gd here), and by exactly twice its size under the inverse-depth
    plane alone, a loss the GPU tests run too."""
    sc = grad_scenes.get("chain")
    orc, ref = _oracle(sc), _ref64(grad_scenes.get("chain"), "planes")
    inv = _ref64(sc, "inv_depth_map")["depths"]
    wrong = ref["depths"] - 2.0 * inv  # the gi term with + for -
    e = gr.rel_err(wrong, ref["depths"])
    print(f"e[depths] with the sign of the gi term flipped: {e:.3f}")
    assert e > 0.1 > 1e3 * pg.bound("depths")
    assert gr.rel_err(-inv, inv) == 2.0


def test_backward_planes_host_abi(tmp_path):
    """gsr_backward_planes is exported and validates before any device call; GsrPlaneGradients is
    laid out as the header's gsr_plane_gradients; the ABI version stays 4."""
    lib = _lib.load_library()
    assert "gsr_backward_planes" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "gsr_backward_planes")
    assert lib.gsr_abi_version() == _lib.ABI_VERSION == 4
    names = [f for f, _ in _lib.GsrPlaneGradients._fields_]
    assert names == ["dL_ddepth_map", "dL_dinv_depth_map", "dL_dfinal_T", "dL_ddepths"]
    probe = tmp_path / "probe.c"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsr.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(gsr_plane_gradients));']
    lines += [f'printf("{f} %zu\\n", offsetof(gsr_plane_gradients, {f}));' for f in names]
    # the structs gsr_backward reads keep their layout (a field added there would be read as garbage)
    lines += ['printf("inputs %zu\\n", sizeof(gsr_backward_inputs));',
              'printf("gradients %zu\\n", sizeof(gsr_gradients));', "return 0;}"]
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(probe), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln}
    assert got["size"] == ctypes.sizeof(_lib.GsrPlaneGradients)
    for f in names:
        assert got[f] == getattr(_lib.GsrPlaneGradients, f).offset, f
    assert got["inputs"] == ctypes.sizeof(_lib.GsrBackwardInputs) == 8
    assert got["gradients"] == ctypes.sizeof(_lib.GsrGradients) == 72

    fn = _lib.backward_planes_fn(lib)
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)  # never dereferenced
    g, st = _lib.GsrGaussians(P=4), _lib.GsrRasterSettings(image_width=8, image_height=8)
    inp, pl, out = _lib.GsrBackwardInputs(), _lib.GsrPlaneGradients(), _lib.GsrGradients()
    ref = ctypes.byref
    for args in ((None, ref(g), ref(st), ref(inp), ref(pl), ref(out)),
                 (ctx, None, ref(st), ref(inp), ref(pl), ref(out)),
                 (ctx, ref(g), None, ref(inp), ref(pl), ref(out)),
                 (ctx, ref(g), ref(st), None, ref(pl), ref(out)),
                 (ctx, ref(g), ref(st), ref(inp), ref(pl), None)):
        assert fn(*args, None) == -1  # GSR_E_INVALID
    st.tile_row_begin, st.tile_row_end = 0, 1
    assert fn(ctx, ref(g), ref(st), ref(inp), ref(pl), ref(out), None) == -1
    assert b"gsr_backward_planes: whole frames only" in lib.gsr_last_error()
    st.tile_row_end = 0
    # no gradient at all, with the struct and without it; dL_ddepths is an output, not a gradient
    assert fn(ctx, ref(g), ref(st), ref(inp), ref(pl), ref(out), None) == -1
    assert b"dL_dcolor or a plane gradient is required" in lib.gsr_last_error()
    pl.dL_ddepths = 64
    assert fn(ctx, ref(g), ref(st), ref(inp), ref(pl), ref(out), None) == -1
    assert fn(ctx, ref(g), ref(st), ref(inp), None, ref(out), None) == -1
    assert b"dL_dcolor is required" in lib.gsr_last_error()
    # one plane gradient stands in for dL_dcolor: the next check is reached
    pl.dL_dfinal_T = 64
    assert fn(ctx, ref(g), ref(st), ref(inp), ref(pl), ref(out), None) == -1
    assert b"SHs or precomputed colors" in lib.gsr_last_error()


def test_depth_maps_setting_is_last_and_off():
    """depth_maps is the settings' last argument, after shading, and defaults to False; upstream's
    constructions hold; _replace carries it.  (It travels beside the tuple: test_shading_reference
    pins the tuple's last field to `shading`.)"""
    import inspect
    params = list(inspect.signature(GaussianRasterizationSettings.__new__).parameters.values())
    assert params[-2].name == "depth_maps" and params[-2].default is False
    upstream = (8, 8, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                False, False)
    rs = GaussianRasterizationSettings(*upstream)
    assert rs.depth_maps is False and rs.shading == 0 and len(rs) == 13
    assert GaussianRasterizationSettings(*upstream, depth_maps=True).depth_maps is True
    assert GaussianRasterizationSettings(*upstream, 0, True).depth_maps is True
    on = rs._replace(depth_maps=True)
    assert on.depth_maps is True and on.shading == 0 and rs.depth_maps is False
    assert on._replace(shading=2).depth_maps is True and on._replace(shading=2).shading == 2
    assert on._replace(depth_maps=False).depth_maps is False
    kw = dict(zip(GaussianRasterizationSettings._fields, upstream))
    assert GaussianRasterizationSettings(**kw, depth_maps=True).depth_maps is True
    with pytest.raises(TypeError):
        GaussianRasterizationSettings(*upstream, 0, True, 1)
