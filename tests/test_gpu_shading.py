"""GPU: the GL shadings (gsr_forward_shaded, csrc/blend.hip k_shade_q) against the float64
reference of shading_reference.py on every scene of shading_scenes.py, in every shading: the
first-hit position and final_T on stable pixels, the colour's bits (billboard, flat ball) or its
bound (gaussian ball) on every pixel; bit-identical under the quadrant cull, GSR_OPT_BLEND_FAST,
the plain call (tight lists where allowed) and strips; then the entry point's argument checks,
frame graphs under alternating shadings, and HIPRenderer(gl_shading=True).
test_shading_reference.py asserts on the CPU that each scene reaches what it was built for."""
import warnings

import numpy as np
import pytest
import torch

from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.camera import Camera
from gaussiansplattingviewer_amd.gaussian_data import synthetic_gaussians
from gaussiansplattingviewer_amd.rasterizer import binning_state, rasterize_gaussians_native
from gaussiansplattingviewer_amd.renderer import HIPRenderer
from gaussiansplattingviewer_amd.strips import strip_pixel_rows

import pose_scenes
import shading_reference as sr
import shading_scenes as ss
from gpu_helpers import set_option, to_dev

pytestmark = pytest.mark.gpu

PIXEL_EXTRAS = ("final_T", "n_contrib")
ALL_EXTRAS = ("depths", "means2D", "conic_opacity", "tiles_touched") + PIXEL_EXTRAS
IMAGES = ("color",) + PIXEL_EXTRAS


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


def _args(sc, dev):
    """The 19 upstream arguments of a scene, on the device."""
    s, g = sc["s"], sc["s"]["g"]
    P = len(g.xyz)
    pre, cov = sc["colors"], sc["cov6"]
    sh = None if pre is not None else to_dev(g.sh.reshape(P, g.sh.shape[-1] // 3, 3), dev)
    return (to_dev(s["bg"], dev), to_dev(g.xyz, dev), to_dev(pre, dev), to_dev(g.opacity, dev),
            to_dev(g.scale, dev) if cov is None else None,
            to_dev(g.rot, dev) if cov is None else None, s["scale_modifier"], to_dev(cov, dev),
            to_dev(s["view"], dev), to_dev(s["proj"], dev), s["tx"], s["ty"], s["H"], s["W"], sh,
            s["sh_degree"], to_dev(s["campos"], dev), False, False)


def _render(sc, dev, shading, extras=ALL_EXTRAS, binning=False, **kw):
    res = rasterize_gaussians_native(*_args(sc, dev), extras=extras, shading=shading, **kw)
    out = {"color": res.color.cpu().numpy(), "num_rendered": res.num_rendered}
    for k, v in res.extras.items():
        out[k] = v.cpu().numpy()
    if "n_contrib" in out:
        out["n_contrib"] = out["n_contrib"].view(np.uint32)
    if binning:
        pl, _, rg = binning_state(dev.index or 0)
        out["point_list"] = pl.cpu().numpy().view(np.uint32)
        out["ranges"] = rg.cpu().numpy().view(np.uint32)
    return out


def _same_bits(a, b, keys, what):
    for k in keys:
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32),
                                      err_msg=f"{what}: {k}")


def _check_against_reference(got, sc, orc, ref, shading, what):
    W, H, bg = sc["W"], sc["H"], sc["s"]["bg"]
    st, nc = ref["stable"], got["n_contrib"].astype(np.int64)
    share = 1.0 - float(st.mean())
    bad = st & (nc != ref["n_contrib"])
    assert not bad.any(), (f"{what}: n_contrib differs at {int(bad.sum())} stable pixels, first "
                           f"(y, x) {tuple(np.argwhere(bad)[0])}")
    # every pixel, stable or not: a position of its list, and final_T and the colour follow it
    assert (nc <= ref["list_len"]).all(), what
    np.testing.assert_array_equal(got["final_T"], np.where(nc > 0, 0.0, 1.0).astype(np.float32),
                                  err_msg=what)
    ent = sr.reported_entry(orc["ranges"], orc["point_list"], orc["means2D"],
                            orc["conic_opacity"], W, H, nc)
    rgb = ref["features"][np.maximum(ent["id"], 0)]  # [H, W, 3] float32
    miss = (nc == 0)[None]
    bg3 = np.broadcast_to(np.asarray(bg, np.float32)[:, None, None], (3, H, W))
    ratio = 0.0
    if shading != sr.GAUSS_BALL:
        want = np.where(miss, bg3, np.moveaxis(rgb, -1, 0))
        np.testing.assert_array_equal(got["color"].view(np.uint32), want.view(np.uint32),
                                      err_msg=f"{what}: colour is not the reported entry's rgb")
    else:
        np.testing.assert_array_equal(got["color"].view(np.uint32)[np.broadcast_to(miss, (3, H, W))],
                                      bg3.view(np.uint32)[np.broadcast_to(miss, (3, H, W))],
                                      err_msg=f"{what}: background")
        hit = nc > 0
        with np.errstate(over="ignore"):
            e = np.exp(ent["power"])
            bound = (np.abs(rgb).max(axis=-1) * e * (np.expm1(ent["dp"]) + 4.0 * sr.U)
                     + 2.0 ** -149)
        err = np.abs(got["color"].astype(np.float64)
                     - np.moveaxis(rgb, -1, 0).astype(np.float64) * e).max(axis=0)
        assert (err[hit] <= bound[hit]).all(), f"{what}: colour beyond the reported entry's bound"
        # and on stable pixels the reference's own colour and bound
        e_ref = np.abs(got["color"].astype(np.float64) - ref["color"]).max(axis=0)
        sh = st & hit
        assert (e_ref[st] <= ref["bound"][st]).all(), f"{what}: stable pixel beyond its bound"
        ratio = float((e_ref[sh] / ref["bound"][sh]).max()) if sh.any() else 0.0
    print(f"{what}: unstable {share:.5f}, hits {float((nc > 0).mean()):.3f}"
          + (f", max err {ratio:.3f} of bound" if shading == sr.GAUSS_BALL else ""))


@pytest.mark.parametrize("name", ss.NAMES)
def test_shading_on_scene(gpu, oracle_mod, scenes, name):
    sc = scenes(name)
    orc = sc["orc"]
    gy = (sc["H"] + 15) // 16
    try:
        for shading in ss.SHADINGS:
            what = f"{name} shading {shading}"
            ref = sr.reference(sc, orc, shading)
            set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 0)
            off = _render(sc, gpu, shading)
            set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 1)
            hip = _render(sc, gpu, shading, binning=True)
            # n_contrib requested: upstream's lists, so positions are upstream's
            assert hip["num_rendered"] == orc["num_rendered"]
            np.testing.assert_array_equal(hip["point_list"], orc["point_list"])
            np.testing.assert_array_equal(hip["ranges"], orc["ranges"])
            for k in ("means2D", "conic_opacity"):
                np.testing.assert_array_equal(hip[k].view(np.uint32), orc[k].view(np.uint32))
            _check_against_reference(hip, sc, orc, ref, shading, what)
            _same_bits(off, hip, IMAGES, what + ": quadrant cull")
            set_option(gpu, _lib.GSR_OPT_BLEND_FAST, 0)
            _same_bits(_render(sc, gpu, shading), hip, IMAGES, what + ": GSR_OPT_BLEND_FAST 0")
            set_option(gpu, _lib.GSR_OPT_BLEND_FAST, 1)
            # the viewer's call: no extras, so tight lists where the shading allows them
            plain = _render(sc, gpu, shading, extras=())
            _same_bits(plain, hip, ("color",), what + ": plain call")
            if gy >= 2:
                for rows in ((0, 1), (1, gy)):
                    y0, n = strip_pixel_rows(rows, sc["H"])
                    full = {k: hip[k][..., y0:y0 + n, :] for k in IMAGES}
                    part = _render(sc, gpu, shading, tile_rows=rows)
                    _same_bits(part, full, IMAGES, f"{what}: strip {rows}")
                    part = _render(sc, gpu, shading, extras=PIXEL_EXTRAS, tile_rows=rows,
                                   radii=False)
                    _same_bits(part, full, IMAGES, f"{what}: strip {rows} without radii")
    finally:
        set_option(gpu, _lib.GSR_OPT_BLEND_FAST, 1)
        set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 1)


@pytest.mark.parametrize("shading", (sr.BILLBOARD, sr.GAUSS_BALL), ids=("billboard", "ball"))
def test_shading_at_the_oblique_pose(gpu, oracle_mod, shading):
    """`mixed` seen from pose_scenes' oblique camera (a dense view rotation; every scene above
    looks through the static camera): one billboard and one ball frame against the same reference
    -- it reads the 2D records, whatever view made them -- under the same bounds."""
    sc = dict(ss.build(oracle_mod, "mixed"))
    view, proj, campos, tx, ty = pose_scenes.camera_inputs(sc["W"], sc["H"], "oblique")
    sc["s"] = dict(sc["s"], view=view, proj=proj, campos=campos, tx=tx, ty=ty)
    orc = ss.run(oracle_mod, sc)
    ref = sr.reference(sc, orc, shading)
    assert 0.2 <= float((ref["n_contrib"] > 0).mean()) < 1.0 and ref["stable"].mean() >= 0.95
    hip = _render(sc, gpu, shading, binning=True)
    assert hip["num_rendered"] == orc["num_rendered"] > 0
    np.testing.assert_array_equal(hip["point_list"], orc["point_list"])
    np.testing.assert_array_equal(hip["ranges"], orc["ranges"])
    for k in ("means2D", "conic_opacity"):
        np.testing.assert_array_equal(hip[k].view(np.uint32), orc[k].view(np.uint32))
    _check_against_reference(hip, sc, orc, ref, shading, f"mixed@oblique shading {shading}")


def test_splat_shading_is_gsr_forward_and_unknown_shadings_are_invalid(gpu, scenes):
    from gaussiansplattingviewer_amd import _C
    sc = scenes("mixed")
    e = torch.empty(0)
    args = tuple(e if a is None else a for a in _args(sc, gpu))
    want = rasterize_gaussians_native(*_args(sc, gpu))  # gsr_forward
    n, color, radii, *_ = _C.rasterize_gaussians_shaded(*args, _lib.GSR_SHADE_SPLAT)
    assert n == want.num_rendered and torch.equal(radii, want.radii)
    assert torch.equal(color.view(torch.int32), want.color.view(torch.int32))
    n, color, radii, *_ = _C.rasterize_gaussians(*args)
    assert torch.equal(color.view(torch.int32), want.color.view(torch.int32))
    for bad in (4, -1):
        with pytest.raises(RuntimeError, match=r"\(-1\).*unknown shading"):
            rasterize_gaussians_native(*_args(sc, gpu), shading=bad)
        with pytest.raises(RuntimeError, match=r"\(-1\).*unknown shading"):
            _C.rasterize_gaussians_shaded(*args, bad)
    # a refused call leaves the context usable
    again = rasterize_gaussians_native(*_args(sc, gpu))
    assert torch.equal(again.color.view(torch.int32), want.color.view(torch.int32))


def test_frame_graphs_under_alternating_shadings(gpu, scenes):
    """Shadings 0, 2, 0, 1 on one context with GSR_OPT_FRAME_GRAPHS 1: every frame equals its
    render without graphs (the recorded chains differ only by the billboard's full lists)."""
    sc = scenes("mixed")
    slot = 46
    args = _args(sc, gpu)  # one set of device tensors: the graphs' key holds their addresses
    ctx = _lib.context(gpu.index or 0, slot)
    before = _lib.get_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS)
    order = (0, 2, 0, 1)
    try:
        _lib.set_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS, 0)
        want = {s: rasterize_gaussians_native(*args, slot=slot, shading=s).color.clone()
                for s in set(order)}
        assert not torch.equal(want[0], want[2]) and not torch.equal(want[1], want[2])
        _lib.set_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS, 1)
        frames0 = _lib.frame_graph_stats(gpu.index or 0, slot)["graph_frames"]
        for s in order + order:  # (the first frame sizes the lists' capacity, the direct way)
            got = rasterize_gaussians_native(*args, slot=slot, shading=s)
            assert torch.equal(got.color.view(torch.int32), want[s].view(torch.int32)), s
        stats = _lib.frame_graph_stats(gpu.index or 0, slot)
        assert stats["graph_frames"] - frames0 >= len(order) and stats["overflows"] == 0
    finally:
        _lib.set_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS, before)
    assert _lib.get_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS) == before


@pytest.mark.parametrize("tile_rows", (None, (1, 4)))
def test_renderer_gl_shading(gpu, tile_rows):
    W, H = 160, 120
    g = synthetic_gaussians(3000, 3, 21)
    cam = Camera(H, W)

    def make(**kw):
        r = HIPRenderer(W, H, device=gpu, tile_rows=tile_rows, **kw)
        r.update_gaussian_data(g)
        r.update_camera_intrin(cam)
        r.update_camera_pose(cam)
        return r

    r = make(gl_shading=True)
    rs, gd = r.raster_settings, r.gaussians
    images = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for mod, shading in ((-2, 1), (-3, 2), (-4, 3)):
            r.set_render_mod(mod)
            got = r.draw()
            want = rasterize_gaussians_native(
                rs["bg"], gd.xyz, None, gd.opacity, gd.scale, gd.rot, rs["scale_modifier"], None,
                rs["viewmatrix"], rs["projmatrix"], rs["tanfovx"], rs["tanfovy"], H, W, gd.sh, 0,
                rs["campos"], False, False, tile_rows=tile_rows, shading=shading).color
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), mod
            images[mod] = got.clone()
        r.set_render_mod(3)
        default = r.draw().clone()
    assert not torch.equal(images[-2], images[-3]) and not torch.equal(images[-3], images[-4])
    assert not torch.equal(images[-3], default)
    # without gl_shading the mode renders the default image, with the one-time warning
    plain = make()
    with pytest.warns(UserWarning, match="GL-only"):
        plain.set_render_mod(-3)
    assert torch.equal(plain.draw().view(torch.int32), default.view(torch.int32))
