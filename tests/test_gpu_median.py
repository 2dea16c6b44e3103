"""The median planes of the blend pass (gsr_forward_surface) on the device.

Accept sets: at every stable pixel of every scene, in both arithmetic modes, median_id is a splat
at which the float64 transmittance crosses 0.5 within the pixel's derived bound (or -1 where it
may stay above), and median_depth is that Gaussian's `depths` bits (median_reference.py; the
float32 restatement alone meets it in test_median_reference.py).  Bit identities (cull, tight
binning, n_contrib, the depth planes, one plane alone; everything else the call returns is
gsr_forward_depth's or gsr_forward's), strips, frame graphs, edges, the NULL struct, and the
renderer's pick and median stereo disparity."""
import ctypes

import numpy as np
import pytest
import torch

from gaussiansplattingviewer_amd import _lib, colmap
from gaussiansplattingviewer_amd.camera import Camera
from gaussiansplattingviewer_amd.gaussian_data import synthetic_gaussians
from gaussiansplattingviewer_amd.rasterizer import binning_state, rasterize_gaussians_native
from gaussiansplattingviewer_amd.renderer import HIPRenderer
from gaussiansplattingviewer_amd.stereo import StereoCapture, median_disparity
from gaussiansplattingviewer_amd.strips import strip_pixel_rows

import depth_scenes as ds
import median_reference as mr
import median_scenes as ms
from gpu_helpers import ALL_EXTRAS, run_hip, set_option, tight_binning, to_dev

pytestmark = pytest.mark.gpu

PLANES = ds.PLANES
SURF = ("median_depth", "median_id")
PIXELS = ("color", "final_T", "n_contrib")
LISTS = ("point_list", "point_tiles", "ranges")
PER_GAUSSIAN = ("radii", "depths", "means2D", "conic_opacity", "rgb", "tiles_touched")


def _render(sc, gpu, extras=ALL_EXTRAS + PLANES + SURF, **kw):
    kw.setdefault("binning", False)
    return run_hip(sc["s"], gpu, colors_precomp=sc["colors"], cov3D_precomp=sc["cov6"],
                   extras=extras, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _same(got, want, keys, what):
    for k in keys:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{what}: {k}")


@pytest.fixture(scope="module")
def scenes(oracle_mod):
    return ms.scene_cache(oracle_mod)


@pytest.fixture
def options(gpu):
    """The context's blend options, restored to their defaults afterwards."""
    try:
        yield lambda opt, v: set_option(gpu, opt, v)
    finally:
        set_option(gpu, _lib.GSR_OPT_BLEND_FAST, 1)
        set_option(gpu, _lib.GSR_OPT_BLEND_CULL, 1)


# ---- 1. accept sets ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ms.NAMES)
def test_median_within_accept_sets(gpu, oracle_mod, scenes, options, name):
    sc = scenes(name)
    orc = sc["orc"]
    ref = mr.reference(oracle_mod, sc, orc)
    mr.assert_scene_decides(ref, name)
    for fast in (1, 0):
        what = f"{name} {'fast' if fast else 'exact'}"
        options(_lib.GSR_OPT_BLEND_FAST, fast)
        hip = _render(sc, gpu, binning=True)
        # the reference walked the oracle's lists: they are this forward's
        _same(hip, orc, ("point_list", "ranges", "depths"), what + " vs oracle")
        mr.assert_median_accepted(ref, sc, hip["median_id"], hip["median_depth"], hip["depths"],
                                  what)
        # and the kernel without n_contrib, on tight lists
        few = _render(sc, gpu, extras=SURF)
        mr.assert_median_accepted(ref, sc, few["median_id"], few["median_depth"], hip["depths"],
                                  what + " (planes only)")


# ---- 2. bit identities ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("layers", "depth_range", "pads_1"))
def test_bit_identities(gpu, scenes, options, name):
    sc = scenes(name)
    for fast in (1, 0):
        what = f"{name} {'fast' if fast else 'exact'}"
        options(_lib.GSR_OPT_BLEND_FAST, fast)
        base = _render(sc, gpu, binning=True)
        assert (base["median_id"] >= 0).any(), what
        # everything else is gsr_forward_depth's ...
        dep = _render(sc, gpu, extras=ALL_EXTRAS + PLANES, binning=True)
        assert base["num_rendered"] == dep["num_rendered"]
        _same(base, dep, PIXELS + PLANES + PER_GAUSSIAN + LISTS, what + " vs gsr_forward_depth")
        # ... and gsr_forward's when no depth plane is asked, on upstream's and on tight lists
        for extras in (ALL_EXTRAS, ()):
            plain = _render(sc, gpu, extras=extras, binning=True)
            surf = _render(sc, gpu, extras=extras + SURF, binning=True)
            assert plain["num_rendered"] == surf["num_rendered"]
            _same(surf, plain, ("color", "radii") + extras + LISTS, what + " vs gsr_forward")
            # with and without n_contrib; with and without the depth planes
            _same(surf, base, SURF, what + f": extras {extras}")
        _same(_render(sc, gpu, extras=PLANES + SURF), base, ("color",) + PLANES + SURF,
              what + ": depth planes, no n_contrib")
        options(_lib.GSR_OPT_BLEND_CULL, 0)
        _same(_render(sc, gpu), base, PIXELS + PLANES + SURF, what + ": no cull")
        _same(_render(sc, gpu, extras=SURF), base, ("color",) + SURF, what + ": no cull, planes only")
        options(_lib.GSR_OPT_BLEND_CULL, 1)
        with tight_binning(gpu, 0):
            _same(_render(sc, gpu, extras=SURF), base, ("color",) + SURF, what + ": tight binning 0")
            _same(_render(sc, gpu, extras=PLANES + SURF), base, ("color",) + PLANES + SURF,
                  what + ": tight binning 0, depth planes")
        for k in SURF:  # one median plane alone
            for more in ((), ALL_EXTRAS + PLANES):
                _same(_render(sc, gpu, extras=more + (k,)), base, ("color", k),
                      what + f": {k} alone")


# ---- 3. strips -----------------------------------------------------------------------------------
def test_strips_have_the_full_frames_rows_and_global_ids(gpu, scenes):
    sc = scenes("layers")
    full = _render(sc, gpu)
    assert (full["median_id"] >= 0).all()
    for rows in ((0, 1), (1, 3), (2, 3)):
        y0, n = strip_pixel_rows(rows, sc["H"])
        want = {k: full[k][..., y0:y0 + n, :] for k in PIXELS + PLANES + SURF}
        _same(_render(sc, gpu, tile_rows=rows), want, PIXELS + PLANES + SURF, f"strip {rows}")
        part = _render(sc, gpu, tile_rows=rows, radii=False, extras=("final_T",) + SURF)
        assert part["radii"] is None and part["median_id"].shape == (n, sc["W"])
        _same(part, want, ("color", "final_T") + SURF, f"strip {rows} without radii")
        # global ids: the strip's medians are the indices of the input tensors
        z = full["depths"][part["median_id"]]
        np.testing.assert_array_equal(_bits(z), _bits(part["median_depth"]))
    assert len(np.unique(full["median_id"][32:])) > 5


# ---- 4. frame graphs -----------------------------------------------------------------------------
def _args(sc, gpu):
    s, g = sc["s"], sc["s"]["g"]
    return (to_dev(s["bg"], gpu), to_dev(g.xyz, gpu), to_dev(sc["colors"], gpu),
            to_dev(g.opacity, gpu), None, None, s["scale_modifier"], to_dev(sc["cov6"], gpu),
            to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["tx"], s["ty"], s["H"], s["W"], None,
            s["sh_degree"], to_dev(s["campos"], gpu), False, False)


def test_frame_graphs_under_alternating_surface_depth_and_plain_forwards(gpu, scenes):
    """Surface, depth and plain forwards of two scenes alternate on one context with
    GSR_OPT_FRAME_GRAPHS 1, then 2: every output equals option 0's bits, and the context records
    exactly the graphs that a context rendering the same scenes with plain frames only records
    (the planes are arguments of the blend's direct launch; nothing of them is in a graph's key)."""
    slot, plain_slot = 149, 150  # (test_gpu_frame_graphs.py: from 20 upwards; 147: the depth maps')
    dev = gpu.index or 0
    two = [(n, _args(scenes(n), gpu)) for n in ("depth_range", "pads_1")]
    extras = {"surface": ("final_T",) + SURF, "both": ("final_T",) + PLANES + SURF,
              "depth": ("final_T",) + PLANES, "plain": ("final_T",)}
    kinds = ("surface", "depth", "plain", "both")

    def frame(args, kind, s):
        r = rasterize_gaussians_native(*args, slot=s, extras=extras[kind])
        return dict(r.extras, color=r.color, radii=r.radii, num_rendered=r.num_rendered)

    def same(got, want, what):
        assert got["num_rendered"] == want["num_rendered"], what
        for k, v in want.items():
            if k != "num_rendered":
                assert torch.equal(got[k].view(torch.int32), v.view(torch.int32)), (what, k)

    def sequence(s, kind_of):
        """Option 0, then 13 frames under each of modes 1 and 2; returns the stats' growth."""
        ctx = _lib.context(dev, s)
        before = _lib.get_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS)
        grown = {}
        try:
            _lib.set_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS, 0)
            want = {(n, k): frame(a, kind_of(k), s) for n, a in two for k in kinds}
            for mode in (1, 2):
                _lib.set_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS, mode)
                s0 = _lib.frame_graph_stats(dev, s)
                # (the first frame sizes the lists' capacity, the direct way)
                for i in range(13):
                    n, a = two[(i // 4) % 2]
                    k = kinds[i % 4]
                    same(frame(a, kind_of(k), s), want[n, k], f"graphs {mode} frame {i} {n} {k}")
                s1 = _lib.frame_graph_stats(dev, s)
                assert s1["overflows"] == 0
                grown[mode] = {k: s1[k] - s0[k] for k in ("graph_frames", "graphs_recorded")}
        finally:
            _lib.set_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS, before)
        assert _lib.get_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS) == before
        return want, grown

    want, mixed = sequence(slot, lambda k: k)
    assert (want["depth_range", "surface"]["median_id"] >= 0).any()
    for n, _ in two:  # (the planes do not depend on what else is asked for)
        same({k: want[n, "both"][k] for k in want[n, "surface"]}, want[n, "surface"], n)
        same({k: want[n, "surface"][k] for k in want[n, "plain"]}, want[n, "plain"], n)
    _, plain = sequence(plain_slot, lambda k: "plain")
    print(f"frame graphs: mixed {mixed}, plain only {plain}")
    assert mixed == plain
    assert mixed[1]["graph_frames"] >= 12 and mixed[2]["graph_frames"] >= 12
    assert mixed[1]["graphs_recorded"] >= 1 and mixed[2]["graphs_recorded"] == 0


# ---- 5. edges ------------------------------------------------------------------------------------
def _c_surface(gpu, args, depth=False, surface="both", guard=0):
    """gsr_forward_surface through ctypes on args (_args): buffers prefilled with a sentinel and
    `guard` more elements behind each plane; surface None = a NULL struct, "empty" = two NULL
    members.  Returns the tensors and num_rendered."""
    bg, xyz, colors, opac, _, _, mod, cov6, view, proj, tx, ty, H, W, _, deg, campos, _, _ = args
    P = xyz.shape[0]
    g = _lib.GsrGaussians(P=P, D=deg, M=0, scale_modifier=mod, means3D=_lib.ptr(xyz),
                          opacities=_lib.ptr(opac), colors_precomp=_lib.ptr(colors),
                          cov3D_precomp=_lib.ptr(cov6))
    st = _lib.GsrRasterSettings(image_width=W, image_height=H, tanfovx=tx, tanfovy=ty,
                                viewmatrix=view.data_ptr(), projmatrix=proj.data_ptr(),
                                campos=campos.data_ptr(), bg=bg.data_ptr())
    t = dict(color=torch.full((3 * H * W + guard,), -7.0, device=gpu),
             radii=torch.zeros(max(P, 1), dtype=torch.int32, device=gpu),
             final_T=torch.full((H * W + guard,), -7.0, device=gpu),
             depth_map=torch.full((H * W + guard,), -7.0, device=gpu),
             inv_depth_map=torch.full((H * W + guard,), -7.0, device=gpu),
             median_depth=torch.full((H * W + guard,), -7.0, device=gpu),
             median_id=torch.full((H * W + guard,), -7, dtype=torch.int32, device=gpu))
    out = _lib.GsrOutputs(color=t["color"].data_ptr(), radii=t["radii"].data_ptr() if P else None,
                          final_T=t["final_T"].data_ptr())
    dp = _lib.GsrDepthOutputs(depth_map=t["depth_map"].data_ptr(),
                              inv_depth_map=t["inv_depth_map"].data_ptr()) if depth else None
    sf = {None: None, "empty": _lib.GsrSurfaceOutputs(),
          "both": _lib.GsrSurfaceOutputs(median_depth=t["median_depth"].data_ptr(),
                                         median_id=t["median_id"].data_ptr())}[surface]
    lib = _lib.load_library()
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    _lib.check(lib.gsr_forward_surface(_lib.context(gpu.index or 0), ctypes.byref(g),
                                       ctypes.byref(st), ctypes.byref(out),
                                       None if dp is None else ctypes.byref(dp),
                                       None if sf is None else ctypes.byref(sf), stream),
               "gsr_forward_surface")
    torch.cuda.synchronize(gpu)
    t["num_rendered"] = out.num_rendered
    return t


def test_no_surface_and_frame_edges(gpu, scenes):
    sc = scenes("ragged_17x9")
    g = sc["s"]["g"]
    H, W = sc["H"], sc["W"]
    behind = dict(sc, s=dict(sc["s"], g=type(g)(g.xyz * np.float32([1, 1, 0]) + np.float32([0, 0, 9]),
                                                 g.rot, g.scale, g.opacity, g.sh)))
    hip = _render(behind, gpu)
    assert hip["num_rendered"] == 0 and not hip["radii"].any()
    assert hip["median_id"].shape == (H, W) and (hip["median_id"] == -1).all()
    assert hip["median_depth"].shape == (H, W) and not _bits(hip["median_depth"]).any()
    empty = dict(behind, s=dict(behind["s"], g=type(g)(g.xyz[:0], g.rot[:0], g.scale[:0],
                                                         g.opacity[:0], g.sh[:0])),
                 colors=sc["colors"][:0], cov6=sc["cov6"][:0])
    hip = _render(empty, gpu, extras=("final_T",) + SURF)
    assert hip["num_rendered"] == 0 and (hip["median_id"] == -1).all()
    assert not _bits(hip["median_depth"]).any()
    # frames that end inside a quadrant (1x1 included): every pixel written, nothing behind them
    for name in ("ragged_1x1", "ragged_7x5", "ragged_9x23", "ragged_17x9"):
        sc = scenes(name)
        n = sc["H"] * sc["W"]
        want = _render(sc, gpu, extras=("final_T",) + PLANES + SURF)
        cases = [sc] + ([dict(sc, s=behind["s"])] if name == "ragged_17x9" else [])
        for case in cases:
            t = _c_surface(gpu, _args(case, gpu), depth=True, guard=64)
            for k in ("color", "final_T", "depth_map", "inv_depth_map", "median_depth", "median_id"):
                m = 3 * n if k == "color" else n
                assert (t[k][m:] == -7).all(), f"{name}: {k} written behind the frame"
                assert not (t[k][:m] == -7).any(), f"{name}: {k} has unwritten pixels"
        t = _c_surface(gpu, _args(sc, gpu), depth=True, guard=64)
        for k in PLANES + SURF + ("final_T",):
            assert np.array_equal(_bits(t[k][:n].cpu().numpy().reshape(sc["H"], sc["W"])),
                                  _bits(want[k])), (name, k)
        ids = want["median_id"]
        assert ((ids == -1) == (want["median_depth"] == 0)).all()
        assert (want["final_T"][ids == -1] > 0.49).all() and (want["final_T"][ids >= 0] < 0.51).all()


# ---- 6. the NULL struct; shadings ----------------------------------------------------------------
def test_null_surface_is_gsr_forward_depth_and_shadings_refuse_the_median(gpu, scenes):
    sc = scenes("depth_range")
    args = _args(sc, gpu)
    H, W = sc["H"], sc["W"]
    want = rasterize_gaussians_native(*args, extras=("final_T",) + PLANES)
    lists = [t.clone() for t in binning_state(gpu.index or 0)]
    plain = rasterize_gaussians_native(*args, extras=("final_T",))
    plain_lists = [t.clone() for t in binning_state(gpu.index or 0)]
    for surface in (None, "empty"):
        for depth, ref, ref_lists in ((True, want, lists), (False, plain, plain_lists)):
            t = _c_surface(gpu, args, depth=depth, surface=surface)
            assert t["num_rendered"] == ref.num_rendered and torch.equal(t["radii"], ref.radii)
            assert torch.equal(t["color"].view(3, H, W).view(torch.int32),
                               ref.color.view(torch.int32))
            for k in ("final_T",) + (PLANES if depth else ()):
                assert torch.equal(t[k].view(H, W).view(torch.int32),
                                   ref.extras[k].view(torch.int32)), k
            for k in SURF + (() if depth else PLANES):  # not touched
                assert (t[k] == -7).all(), k
            for a, b in zip(binning_state(gpu.index or 0), ref_lists):
                assert torch.equal(a, b)
    for shading in (1, 2, 3):
        for k in SURF:
            with pytest.raises(RuntimeError, match="splat composite"):
                rasterize_gaussians_native(*args, extras=(k,), shading=shading)
    with pytest.raises(ValueError, match="unknown extra"):
        rasterize_gaussians_native(*args, extras=("median",))


# ---- 7. the renderer: pick and the median disparity ----------------------------------------------
POSE = ["2", "0.9962", "0", "0.0872", "0", "0.3", "-0.1", "4.5", "1", "b.png"]
W7, H7 = 192, 96


def _layers_viewer_scene(cam):
    """`layers` in the left view of POSE: wall, veil and foreground Gaussians (isotropic, SH
    degree 0) by view depth, left pixel centre and sigma in pixels."""
    rng = np.random.default_rng(7)
    left, _ = colmap.load_camera_positions(POSE)
    inv = np.linalg.inv(left["camera_view"].astype(np.float64))
    tx, ty, _ = cam.get_htanfovxy_focal()
    fx, fy = W7 / (2 * tx), H7 / (2 * ty)
    nw, nv, nf = 16, 24, 60
    px = np.concatenate([rng.uniform(0, W7, nw), rng.uniform(0, W7, nv), rng.uniform(8, W7 - 8, nf)])
    py = np.concatenate([rng.uniform(0, H7, nw), rng.uniform(0, H7, nv), rng.uniform(8, H7 - 8, nf)])
    d = np.concatenate([rng.uniform(8.0, 8.5, nw), rng.uniform(4.0, 4.4, nv), rng.uniform(1.0, 2.0, nf)])
    sigma = np.concatenate([np.full(nw, 60.0), rng.uniform(8, 14, nv), rng.uniform(2, 6, nf)])
    opac = np.concatenate([np.full(nw, 0.9), np.full(nv, 0.3), rng.uniform(0.6, 0.95, nf)])
    n = nw + nv + nf
    g = synthetic_gaussians(n, 3, 33)
    for i in range(n):
        xv, yv = (px[i] - (W7 - 1) / 2) * d[i] / fx, -(py[i] - (H7 - 1) / 2) * d[i] / fy
        g.xyz[i] = (inv @ np.array([xv, yv, -d[i], 1.0]))[:3]
        g.scale[i] = sigma[i] * d[i] / fx
    g.rot[:] = np.float32([1, 0, 0, 0])
    g.opacity[:] = opac.reshape(-1, 1).astype(np.float32)
    g.sh[:] = 0
    g.sh[:, :3] = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    return g


def test_renderer_pick_and_median_stereo_capture(gpu):
    cam = Camera(H7, W7)
    g = _layers_viewer_scene(cam)
    r = HIPRenderer(W7, H7, device=gpu, surface_maps=True)
    r.update_gaussian_data(g)
    frames = StereoCapture(r, cam, disparity="median").render(POSE)
    assert set(frames) == {"left", "right", "disparity"} and r.surface_maps
    disp = frames["disparity"]
    assert disp.dtype == torch.float32 and disp.shape == (H7, W7)
    assert r.depth_map is None and r.inv_depth_map is None  # (depth_maps is its own keyword)
    # the planes left in the renderer are the left frame's
    ids, zmed = r.median_id, r.median_depth
    assert ids.dtype == torch.int32 and ids.shape == (H7, W7) and zmed.shape == (H7, W7)
    rs = r.raster_settings
    assert torch.equal(disp, median_disparity(zmed, rs["tanfovx"], W7))
    # the left pose's per-Gaussian depths
    left_pose, _ = colmap.load_camera_positions(POSE)
    r.update_camera_pose(cam, True, left_pose)
    rs = r.raster_settings
    res = rasterize_gaussians_native(rs["bg"], r.gaussians.xyz, None, r.gaussians.opacity,
                                     r.gaussians.scale, r.gaussians.rot, 1.0, None,
                                     rs["viewmatrix"], rs["projmatrix"], rs["tanfovx"],
                                     rs["tanfovy"], H7, W7, r.gaussians.sh, rs["sh_degree"],
                                     rs["campos"], False, False, extras=("depths",) + SURF)
    assert torch.equal(res.extras["median_id"], ids)
    z = res.extras["depths"].cpu().numpy()
    ids_h, disp_h = ids.cpu().numpy(), disp.cpu().numpy()
    assert (ids_h >= 0).mean() > 0.9 and len(np.unique(ids_h)) > 30
    # every disparity is bitwise fx |B| / z_i of one Gaussian, or 0
    scale = np.float32(W7 / (2.0 * rs["tanfovx"]) * abs(colmap.BASELINE))
    cand = np.concatenate([(scale / z[z > 0]).astype(np.float32), np.float32([0])])
    assert np.isin(_bits(disp_h), _bits(cand)).all()
    want = np.where(ids_h >= 0, scale / np.where(ids_h >= 0, z[np.maximum(ids_h, 0)], 1), 0)
    np.testing.assert_array_equal(_bits(disp_h), _bits(want.astype(np.float32)))
    # none lies between the layers' disparities; the metric (expected) disparity does
    def between(d):
        d = d.astype(np.float64)
        out = np.zeros(d.shape, bool)
        for lo, hi in ms.GAPS:
            out |= (d > scale / hi) & (d < scale / lo)
        return out
    assert not between(disp_h).any()
    rm = HIPRenderer(W7, H7, device=gpu, depth_maps=True)
    rm.update_gaussian_data(g)
    metric = StereoCapture(rm, cam, disparity="metric").render(POSE)
    mixed = between(metric["disparity"].cpu().numpy())
    print(f"between the layers: median 0, metric {int(mixed.sum())} of {mixed.size} pixels")
    assert mixed.sum() > 100
    assert torch.equal(metric["left"], frames["left"]) and torch.equal(metric["right"], frames["right"])
    # pick: one element of median_id; -1 off-surface and outside the frame
    for y, x in ((0, 0), (H7 // 2, W7 // 2), (H7 - 1, W7 - 1), (17, 101), (60, 33)):
        assert r.pick(x, y) == int(ids_h[y, x])
    assert r.pick(-1, 0) == -1 and r.pick(W7, 0) == -1 and r.pick(0, H7) == -1
    # the same Gaussians at opacity 0.004: no transmittance reaches 0.5, no surface anywhere
    faint = HIPRenderer(W7, H7, device=gpu, surface_maps=True)
    faint.update_gaussian_data(type(g)(g.xyz, g.rot, g.scale, np.full_like(g.opacity, 0.004), g.sh))
    with pytest.raises(RuntimeError, match="drawn frame"):
        faint.pick(0, 0)
    faint.update_camera_intrin(cam)
    faint.update_camera_pose(cam, True, left_pose)
    faint.draw()
    assert (faint.median_id == -1).all() and not faint.median_depth.any()
    assert faint.pick(W7 // 2, H7 // 2) == -1 and faint.pick(0, 0) == -1
    # the default modes are unchanged by the keyword, and a renderer without it has no pick
    plain = HIPRenderer(W7, H7, device=gpu)
    plain.update_gaussian_data(g)
    want = StereoCapture(plain, cam).render(POSE)
    assert plain.median_id is None and plain.median_depth is None
    gl = StereoCapture(r, cam, disparity="gl").render(POSE)
    assert set(gl) == {"left", "depth", "right"}
    for k in ("left", "depth", "right"):
        assert torch.equal(gl[k], want[k]), k
    for k in ("left", "right"):
        assert torch.equal(frames[k], want[k]), k
    with pytest.raises(RuntimeError, match="surface_maps=True"):
        plain.pick(0, 0)
    with pytest.raises(RuntimeError, match="surface_maps=True"):
        StereoCapture(plain, cam, disparity="median")
    # a GL shading composites nothing: no median planes, pick -1
    shaded = HIPRenderer(W7, H7, device=gpu, gl_shading=True, surface_maps=True)
    shaded.update_gaussian_data(g)
    shaded.update_camera_intrin(cam)
    shaded.update_camera_pose(cam, True, left_pose)
    shaded.set_render_mod(-3)
    shaded.draw()
    assert shaded.median_id is None and shaded.median_depth is None and shaded.pick(5, 5) == -1
    shaded.set_render_mod(3)
    shaded.draw()
    assert torch.equal(shaded.median_id, ids)
