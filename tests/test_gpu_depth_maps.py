"""The depth planes of the blend pass (gsr_forward_depth) on the device.

Twin: each plane is, bit for bit, a colour channel of an ordinary forward of the same scene with
colors_precomp = (z, 1 / z, 0) and bg = 0, in both arithmetic modes, and everything else the
depth forward returns is the plain forward's.  Float64: the planes meet, per pixel, the bound of
oracle.render_f64 on the same features (depth_scenes.assert_plane_exact; the oracle alone meets
it in test_depth_maps_host.py).  Invariances (cull, tight binning, one plane, the paired-slot
kernel, strips), edges, frame graphs, and the stereo capture's metric disparity against the
pose's geometry."""
import ctypes

import numpy as np
import pytest
import torch

from gaussiansplattingviewer_amd import _lib, colmap
from gaussiansplattingviewer_amd.camera import Camera
from gaussiansplattingviewer_amd.gaussian_data import synthetic_gaussians
from gaussiansplattingviewer_amd.pipeline import FramePipeline
from gaussiansplattingviewer_amd.rasterizer import binning_state, rasterize_gaussians_native
from gaussiansplattingviewer_amd.renderer import HIPRenderer
from gaussiansplattingviewer_amd.stereo import StereoCapture, metric_disparity
from gaussiansplattingviewer_amd.strips import strip_pixel_rows

import blend_scenes as bs
import depth_scenes as ds
from gpu_helpers import ALL_EXTRAS, assert_parity, run_hip, set_option, tight_binning, to_dev

pytestmark = pytest.mark.gpu

PLANES = ds.PLANES
PIXELS = ("color", "final_T", "n_contrib")


def _render(sc, gpu, extras=ALL_EXTRAS + PLANES, **kw):
    kw.setdefault("binning", False)
    return run_hip(sc["s"], gpu, colors_precomp=sc["colors"], cov3D_precomp=sc["cov6"],
                   extras=extras, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, keys, what):
    for k in keys:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{what}: {k}")


@pytest.fixture(scope="module")
def scenes(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            sc = ds.build(oracle_mod, name)
            bs.run(oracle_mod, sc)
            cache[name] = sc
        return cache[name]
    return get


@pytest.mark.parametrize("name", ds.NAMES)
def test_planes_on_edge_scene(gpu, oracle_mod, scenes, name):
    sc = scenes(name)
    orc = sc["orc"]
    ref = ds.reference(oracle_mod, sc, orc)
    gy = (sc["H"] + 15) // 16
    try:
        for fast in (1, 0):
            what = f"{name} {'fast' if fast else 'exact'}"
            set_option(gpu, _lib.GSR_OPT_BLEND_FAST, fast)
            set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 1)
            plain = _render(sc, gpu, extras=ALL_EXTRAS, binning=True)
            hip = _render(sc, gpu, binning=True)
            # 1. everything else is the plain forward's ...
            assert hip["num_rendered"] == plain["num_rendered"]
            _same(hip, plain, PIXELS + ("radii", "depths", "means2D", "conic_opacity", "rgb",
                                        "tiles_touched", "point_list", "point_tiles", "ranges"),
                  what + " depth vs plain forward")
            assert_parity(hip, orc, image=False)  # (and the oracle's: its lists are the reference's)
            # ... and the planes are channels 0 and 1 of the twin forward
            z, iz = ds.features(hip["depths"], hip["radii"])
            twin = run_hip(ds.zero_bg(sc), gpu, binning=False, cov3D_precomp=sc["cov6"],
                           colors_precomp=np.stack([z, iz, np.zeros_like(z)], axis=1))
            np.testing.assert_array_equal(_bits(hip["depth_map"]), _bits(twin["color"][0]),
                                          err_msg=what + ": depth_map is not its twin channel")
            np.testing.assert_array_equal(_bits(hip["inv_depth_map"]), _bits(twin["color"][1]),
                                          err_msg=what + ": inv_depth_map is not its twin channel")
            _same(twin, plain, ("final_T", "n_contrib"), what + " twin")
            # 2. float64 bound
            for k in PLANES:
                assert hip[k].shape == (sc["H"], sc["W"]) and hip[k].dtype == np.float32
                ds.assert_plane_exact(hip[k], hip["n_contrib"], ref[k], f"{what} {k}")
            # 3. invariances, as bits
            set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 0)
            _same(_render(sc, gpu), hip, PIXELS + PLANES, what + ": no cull")
            set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 1)
            for k in PLANES:  # one plane requested
                one = _render(sc, gpu, extras=ALL_EXTRAS + (k,))
                _same(one, hip, PIXELS + (k,), what + f": {k} alone")
            # no other extras: the paired-slot kernel on tight lists, then on upstream's
            few = _render(sc, gpu, extras=PLANES)
            _same(few, hip, ("color",) + PLANES, what + ": planes only (tight lists)")
            with tight_binning(gpu, 0):
                _same(_render(sc, gpu, extras=PLANES), few, ("color",) + PLANES,
                      what + ": tight binning 0")
            if gy >= 2:
                for rows in ((0, 1), (1, gy)):
                    y0, n = strip_pixel_rows(rows, sc["H"])
                    full = {k: hip[k][..., y0:y0 + n, :] for k in PIXELS + PLANES}
                    _same(_render(sc, gpu, tile_rows=rows), full, PIXELS + PLANES,
                          what + f": strip {rows}")
                    part = _render(sc, gpu, tile_rows=rows, radii=False,
                                   extras=("final_T",) + PLANES)
                    assert part["radii"] is None
                    _same(part, full, ("color", "final_T") + PLANES,
                          what + f": strip {rows} without radii")
    finally:
        set_option(gpu, _lib.GSR_OPT_BLEND_FAST, 1)
        set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 1)


def test_planes_differ_by_what_they_should(gpu, scenes):
    """depth_range: the two planes are not each other (nor a constant multiple), and debug mode
    renders the same bits."""
    sc = scenes("depth_range")
    hip = _render(sc, gpu)
    d, i = hip["depth_map"].astype(np.float64), hip["inv_depth_map"].astype(np.float64)
    cover = 1.0 - hip["final_T"].astype(np.float64)
    on = cover > 0.5
    assert on.sum() > 500
    # expected depth and expected inverse depth of a pixel lie within the scene's range, and by
    # Jensen E[z] E[1/z] >= 1 (with margin for rounding), far above 1 where depths mix
    ez, eiz = d[on] / cover[on], i[on] / cover[on]
    assert ez.min() > 0.29 and ez.max() < 51 and eiz.min() > 1 / 51 and eiz.max() < 1 / 0.29
    assert (ez * eiz >= 1 - 1e-5).all() and (ez * eiz).max() > 2
    _same(_render(sc, gpu, debug=True), hip, PIXELS + PLANES, "debug")


def test_all_gaussians_behind_the_camera(gpu, scenes):
    sc = scenes("ragged_17x9")
    g = sc["s"]["g"]
    behind = dict(sc, s=dict(sc["s"], g=type(g)(g.xyz * np.float32([1, 1, 0]) + np.float32([0, 0, 9]),
                                                 g.rot, g.scale, g.opacity, g.sh)))
    hip = _render(behind, gpu)
    assert hip["num_rendered"] == 0 and not hip["radii"].any()
    for k in PLANES:
        assert hip[k].shape == (sc["H"], sc["W"]) and not _bits(hip[k]).any(), k
    assert (hip["final_T"] == 1).all()
    empty = dict(behind, s=dict(behind["s"], g=type(g)(g.xyz[:0], g.rot[:0], g.scale[:0],
                                                         g.opacity[:0], g.sh[:0])),
                 colors=sc["colors"][:0], cov6=sc["cov6"][:0])
    hip = _render(empty, gpu, extras=("final_T",) + PLANES)
    assert hip["num_rendered"] == 0
    for k in PLANES:
        assert not _bits(hip[k]).any(), k


def _args(sc, gpu):
    s, g = sc["s"], sc["s"]["g"]
    return (to_dev(s["bg"], gpu), to_dev(g.xyz, gpu), to_dev(sc["colors"], gpu),
            to_dev(g.opacity, gpu), None, None, s["scale_modifier"], to_dev(sc["cov6"], gpu),
            to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["tx"], s["ty"], s["H"], s["W"], None,
            s["sh_degree"], to_dev(s["campos"], gpu), False, False)


def test_null_planes_are_gsr_forward_and_shadings_refuse_planes(gpu, scenes):
    sc = scenes("depth_range")
    args = _args(sc, gpu)
    want = rasterize_gaussians_native(*args, extras=("final_T",))
    lists = [t.clone() for t in binning_state(gpu.index or 0)]
    # the C entry point with a NULL struct and with two NULL planes
    bg, xyz, colors, opac, _, _, mod, cov6, view, proj, tx, ty, H, W, _, deg, campos, _, _ = args
    P = xyz.shape[0]
    g = _lib.GsrGaussians(P=P, D=deg, M=0, scale_modifier=mod, means3D=xyz.data_ptr(),
                          opacities=opac.data_ptr(), colors_precomp=colors.data_ptr(),
                          cov3D_precomp=cov6.data_ptr())
    st = _lib.GsrRasterSettings(image_width=W, image_height=H, tanfovx=tx, tanfovy=ty,
                                viewmatrix=view.data_ptr(), projmatrix=proj.data_ptr(),
                                campos=campos.data_ptr(), bg=bg.data_ptr())
    lib = _lib.load_library()
    ctx = _lib.context(gpu.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    for planes in (None, _lib.GsrDepthOutputs()):
        color = torch.full((3, H, W), -1.0, device=gpu)
        radii = torch.zeros(P, dtype=torch.int32, device=gpu)
        final_T = torch.full((H, W), -1.0, device=gpu)
        out = _lib.GsrOutputs(color=color.data_ptr(), radii=radii.data_ptr(),
                              final_T=final_T.data_ptr())
        _lib.check(lib.gsr_forward_depth(ctx, ctypes.byref(g), ctypes.byref(st), ctypes.byref(out),
                                         None if planes is None else ctypes.byref(planes), stream),
                   "gsr_forward_depth")
        assert out.num_rendered == want.num_rendered and torch.equal(radii, want.radii)
        assert torch.equal(color.view(torch.int32), want.color.view(torch.int32))
        assert torch.equal(final_T.view(torch.int32), want.extras["final_T"].view(torch.int32))
        for a, b in zip(binning_state(gpu.index or 0), lists):
            assert torch.equal(a, b)
    for shading in (1, 2, 3):
        with pytest.raises(RuntimeError, match="splat composite"):
            rasterize_gaussians_native(*args, extras=("depth_map",), shading=shading)
    with pytest.raises(ValueError, match="unknown extra"):
        rasterize_gaussians_native(*args, extras=("depth",))


def test_frame_graphs_under_alternating_depth_and_plain_forwards(gpu, scenes):
    """Depth and plain forwards of two scenes alternate on one context with GSR_OPT_FRAME_GRAPHS
    1, then 2: every output equals option 0's bits (the planes are arguments of the blend's
    direct launch; nothing of them is recorded, no plane is left unwritten)."""
    slot = 147  # (test_gpu_frame_graphs.py hands out slots from 20 upwards)
    dev = gpu.index or 0
    ctx = _lib.context(dev, slot)
    before = _lib.get_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS)
    two = [(n, _args(scenes(n), gpu)) for n in ("depth_range", "pads_1")]
    extras = {True: ("final_T",) + PLANES, False: ("final_T",)}

    def frame(args, depth, s=slot):
        r = rasterize_gaussians_native(*args, slot=s, extras=extras[depth])
        return dict(r.extras, color=r.color, radii=r.radii, num_rendered=r.num_rendered)

    def same(got, want, what):
        assert got["num_rendered"] == want["num_rendered"], what
        for k, v in want.items():
            if k != "num_rendered":
                assert torch.equal(got[k].view(torch.int32), v.view(torch.int32)), (what, k)

    try:
        _lib.set_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS, 0)
        want = {(n, d): frame(a, d) for n, a in two for d in (True, False)}
        assert want["depth_range", True]["depth_map"].max() > 0
        for mode in (1, 2):
            _lib.set_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS, mode)
            frames0 = _lib.frame_graph_stats(dev, slot)["graph_frames"]
            # (the first frame sizes the lists' capacity, the direct way)
            for i in range(9):
                n, a = two[(i // 2) % 2]
                d = i % 2 == 0
                same(frame(a, d), want[n, d], f"graphs {mode} frame {i} {n} depth={d}")
            stats = _lib.frame_graph_stats(dev, slot)
            assert stats["graph_frames"] - frames0 >= 8 and stats["overflows"] == 0
    finally:
        _lib.set_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS, before)
    assert _lib.get_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS) == before
    # frames in flight: depth frames on the pipeline's streams and context slots
    n, a = two[0]
    with FramePipeline(depth=2, device=gpu) as pipe:
        got = []
        for _ in range(2):
            with pipe.frame() as s:
                got.append(frame(a, True, s))
        pipe.synchronize()
    for g in got:
        same(g, want[n, True], "FramePipeline(depth=2)")


# ---- the stereo capture's metric disparity against the pose's geometry --------------------------
POSE = ["2", "0.9962", "0", "0.0872", "0", "0.3", "-0.1", "4.5", "1", "b.png"]
W6, H6 = 320, 144
# view depth, left pixel centre (x, y): apart on screen in both views (x_right = x_left - d)
SPOTS = ((1.0, 250.3, 70.2), (2.0, 100.6, 100.4), (4.0, 200.1, 125.7), (8.0, 60.5, 20.0),
         (16.0, 290.8, 40.3))


def _stereo_scene(cam):
    """Five small opaque Gaussians at SPOTS in the left view (sigma 1.5 px), white."""
    left, _ = colmap.load_camera_positions(POSE)
    inv = np.linalg.inv(left["camera_view"].astype(np.float64))
    tx, ty, _ = cam.get_htanfovxy_focal()
    fx, fy = W6 / (2 * tx), H6 / (2 * ty)
    g = synthetic_gaussians(len(SPOTS), 3, 31)
    for i, (d, px, py) in enumerate(SPOTS):
        xv, yv = (px - (W6 - 1) / 2) * d / fx, -(py - (H6 - 1) / 2) * d / fy
        g.xyz[i] = (inv @ np.array([xv, yv, -d, 1.0]))[:3]
        g.scale[i] = 1.5 * d / fx
    g.rot[:] = np.float32([1, 0, 0, 0])
    g.opacity[:] = 0.95
    g.sh[:] = 0
    g.sh[:, :3] = 1.0
    return g


def test_metric_disparity_of_the_stereo_capture(gpu):
    cam = Camera(H6, W6)
    g = _stereo_scene(cam)
    r = HIPRenderer(W6, H6, device=gpu, depth_maps=True)
    r.update_gaussian_data(g)
    cap = StereoCapture(r, cam, disparity="metric")
    frames = cap.render(POSE)
    assert set(frames) == {"left", "right", "disparity"}
    disp = frames["disparity"]
    assert disp.dtype == torch.float32 and disp.shape == (H6, W6)
    assert r.depth_maps and r.inv_depth_map is not None and r.final_T.shape == (H6, W6)
    assert torch.equal(disp, metric_disparity(r.inv_depth_map, r.final_T,
                                              r.raster_settings["tanfovx"], W6))
    disp = disp.cpu().numpy()
    right = frames["right"].cpu().numpy().astype(np.int64).sum(axis=2)
    # the poses in float64: view-space z and the left pixel centre of every Gaussian
    left_pose, _ = colmap.load_camera_positions(POSE)
    r.update_camera_pose(cam, True, left_pose)
    vm = r.raster_settings["viewmatrix"].cpu().numpy().T.astype(np.float64)
    pm = r.raster_settings["projmatrix"].cpu().numpy().T.astype(np.float64)
    fx = W6 / (2.0 * r.raster_settings["tanfovx"])
    for i, (d, px, py) in enumerate(SPOTS):
        p = np.append(g.xyz[i].astype(np.float64), 1.0)
        z = (vm @ p)[2]
        ph = pm @ p
        cx, cy = ((ph[0] / ph[3] + 1) * W6 - 1) / 2, ((ph[1] / ph[3] + 1) * H6 - 1) / 2
        assert abs(z - d) < 1e-4 and abs(cx - px) < 0.01 and abs(cy - py) < 0.01
        want = fx * abs(colmap.BASELINE) / z
        got = disp[int(round(cy)), int(round(cx))]
        print(f"z {z:.6f}: disparity {got:.6f}, fx |B| / z {want:.6f}, rel {abs(got - want) / want:.2e}")
        assert abs(got - want) <= 1e-5 * want, (i, got, want)
        band = right[int(round(cy)) - 4:int(round(cy)) + 5]
        assert band.max() > 300
        x_right = np.unravel_index(band.argmax(), band.shape)[1]
        assert abs(x_right - (cx - want)) <= 1.0, (i, x_right, cx - want)
    # no surface: 0; the saved PNG is the KITTI encoding
    assert disp[0, 0] == 0.0 and (disp >= 0).all()


def test_capture_modes_agree_with_the_default(gpu, tmp_path):
    cam = Camera(H6, W6)
    g = synthetic_gaussians(4000, 3, 32)
    plain = HIPRenderer(W6, H6, device=gpu)
    plain.update_gaussian_data(g)
    want = StereoCapture(plain, cam).render(POSE)
    assert plain.depth_map is None and plain.final_T is None
    r = HIPRenderer(W6, H6, device=gpu, depth_maps=True)
    r.update_gaussian_data(g)
    gl = StereoCapture(r, cam, disparity="gl").render(POSE)
    assert set(gl) == {"left", "depth", "right"}
    both = StereoCapture(r, cam, disparity="both").render(POSE)
    metric = StereoCapture(r, cam, disparity="metric").render(POSE)
    assert set(both) == {"left", "depth", "right", "disparity"}
    for k in ("left", "depth", "right"):
        assert torch.equal(gl[k], want[k]) and torch.equal(both[k], want[k]), k
    for k in ("left", "right"):
        assert torch.equal(metric[k], want[k]), k
    assert torch.equal(metric["disparity"], both["disparity"]) and r.depth_maps
    with pytest.raises(RuntimeError, match="depth_maps=True"):
        StereoCapture(plain, cam, disparity="metric")
    # GL shadings composite nothing: no planes
    shaded = HIPRenderer(W6, H6, device=gpu, gl_shading=True, depth_maps=True)
    shaded.update_gaussian_data(g)
    shaded.update_camera_intrin(cam)
    shaded.update_camera_pose(cam)
    shaded.set_render_mod(-3)
    shaded.draw()
    assert shaded.depth_map is None and shaded.inv_depth_map is None and shaded.final_T is None
    shaded.set_render_mod(3)
    shaded.draw()
    assert shaded.depth_map.shape == (H6, W6)
    # strips: strip-local planes
    strip = HIPRenderer(W6, H6, device=gpu, tile_rows=(2, 5), depth_maps=True)
    strip.update_gaussian_data(g)
    strip.update_camera_intrin(cam)
    strip.update_camera_pose(cam)
    strip.draw()
    assert torch.equal(strip.inv_depth_map.view(torch.int32),
                       shaded.inv_depth_map[32:80].view(torch.int32))
    paths = StereoCapture.save(both, str(tmp_path), "scene", 7)
    from PIL import Image
    assert [p.split("/")[-2] for p in paths] == ["left", "depth", "disparity", "right"]
    png = np.array(Image.open(paths[2]))
    d = both["disparity"].cpu().numpy().astype(np.float64)
    assert png.dtype == np.uint16 and png.shape == (H6, W6)
    np.testing.assert_array_equal(png, np.minimum(65535, np.rint(256 * d)).astype(np.uint16))
    assert (png[d == 0] == 0).all() and png.max() > 0
