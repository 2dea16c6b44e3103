"""GPU: frames in flight (FramePipeline: context slots on streams of their own, each frame on
one stream or with its second stream) render every frame bit-identically to serial forwards,
on a moving camera (per-frame re-sort), full frames and strips; and the oracle agrees with the
pipelined frames."""
import numpy as np
import pytest
import torch

from gaussiansplattingviewer_amd.camera import cuda_camera_inputs, orbit_eye, static_camera
from gaussiansplattingviewer_amd.gaussian_data import synthetic_gaussians
from gaussiansplattingviewer_amd.pipeline import FramePipeline
from gaussiansplattingviewer_amd.rasterizer import rasterize_gaussians_native

from gpu_helpers import assert_image_close

pytestmark = pytest.mark.gpu


def _scene(dev, P, W, H, n_frames, seed):
    g = synthetic_gaussians(P, 3, seed)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dev_g = dict(xyz=up(g.xyz), rot=up(g.rot), scale=up(g.scale), opacity=up(g.opacity),
                 sh=up(g.sh).reshape(P, -1, 3).contiguous())
    cams = []
    for i in range(n_frames):
        view, proj, campos, tx, ty = cuda_camera_inputs(static_camera(W, H, orbit_eye(i * 37, 1000)))
        cams.append(dict(view=up(view), proj=up(proj), campos=up(campos), tx=tx, ty=ty,
                         host=(view, proj, campos)))
    return g, dev_g, cams


def _render(dg, cam, W, H, dev, slot=0, tile_rows=None):
    return rasterize_gaussians_native(
        torch.zeros(3, device=dev), dg["xyz"], None, dg["opacity"], dg["scale"], dg["rot"], 1.0,
        None, cam["view"], cam["proj"], cam["tx"], cam["ty"], H, W, dg["sh"], 3, cam["campos"],
        False, False, slot=slot, tile_rows=tile_rows)


# (depth >= 3 runs each frame on one stream, GSR_OPT_SECOND_STREAM 0; second_stream forces it)
@pytest.mark.parametrize("depth,tile_rows,graphs,second_stream",
                         [(2, None, False, None), (3, None, False, None), (4, None, False, None),
                          (4, (3, 9), False, None), (2, None, False, False),
                          (4, None, False, True), (2, (3, 9), False, None),
                          (2, None, True, None), (2, (3, 9), True, None)])
def test_pipelined_frames_equal_serial(gpu, depth, tile_rows, graphs, second_stream):
    P, W, H, n = 60_000, 640, 480, 9
    _, dg, cams = _scene(gpu, P, W, H, n, seed=11)
    serial = []
    for cam in cams:
        r = _render(dg, cam, W, H, gpu, tile_rows=tile_rows)
        serial.append((r.num_rendered, r.color.clone(), r.radii.clone()))
    torch.cuda.synchronize()

    pipe = FramePipeline(depth, gpu, graphs=graphs, second_stream=second_stream)
    assert pipe.second_stream == (second_stream if second_stream is not None
                                  else depth < 3 or graphs)
    piped = []
    for cam in cams:
        with pipe.frame() as slot:
            r = _render(dg, cam, W, H, gpu, slot=slot, tile_rows=tile_rows)
            piped.append((r.num_rendered, r.color, r.radii))
    torch.cuda.synchronize()
    # (later tests see direct launches on two streams again)
    FramePipeline(depth, gpu, graphs=False, second_stream=True)
    for (k0, c0, r0), (k1, c1, r1) in zip(serial, piped):
        assert k0 == k1
        assert torch.equal(r0, r1)
        assert torch.equal(c0.view(torch.int32), c1.view(torch.int32))  # bit-identical


def test_pipelined_frames_match_oracle(gpu, oracle_mod):
    P, W, H, n = 20_000, 320, 240, 4
    g, dg, cams = _scene(gpu, P, W, H, n, seed=5)
    pipe = FramePipeline(2, gpu)
    got = []
    for cam in cams:
        with pipe.frame() as slot:
            got.append(_render(dg, cam, W, H, gpu, slot=slot).color)
    torch.cuda.synchronize()
    for cam, color in zip(cams, got):
        view, proj, campos = cam["host"]
        want = oracle_mod.forward(g.xyz, g.opacity, view, proj, campos, cam["tx"], cam["ty"], W,
                                  H, shs=g.sh, sh_degree=3, scales=g.scale,
                                  rotations=g.rot)["color"]
        assert_image_close(color.cpu().numpy(), want)


def test_pipeline_out_color_buffer(gpu):
    """Rendering into a preallocated buffer (the strip gather's send view) equals a fresh one."""
    P, W, H = 30_000, 320, 240
    _, dg, cams = _scene(gpu, P, W, H, 1, seed=3)
    ref = _render(dg, cams[0], W, H, gpu).color
    buf = torch.full((3 * H * W + 100,), float("nan"), device=gpu)
    view = buf[:3 * H * W].view(3, H, W)
    out = rasterize_gaussians_native(
        torch.zeros(3, device=gpu), dg["xyz"], None, dg["opacity"], dg["scale"], dg["rot"], 1.0,
        None, cams[0]["view"], cams[0]["proj"], cams[0]["tx"], cams[0]["ty"], H, W, dg["sh"], 3,
        cams[0]["campos"], False, False, out_color=view)
    torch.cuda.synchronize()
    assert out.color.data_ptr() == view.data_ptr()
    assert torch.equal(ref.view(torch.int32), view.view(torch.int32))
    assert torch.isnan(buf[3 * H * W:]).all()
    with pytest.raises(RuntimeError):
        _ = rasterize_gaussians_native(
            torch.zeros(3, device=gpu), dg["xyz"], None, dg["opacity"], dg["scale"], dg["rot"],
            1.0, None, cams[0]["view"], cams[0]["proj"], cams[0]["tx"], cams[0]["ty"], H, W,
            dg["sh"], 3, cams[0]["campos"], False, False, out_color=buf[:3 * H * W].view(3, W, H))


def test_second_stream_option(gpu):
    """GSR_OPT_SECOND_STREAM: 0 / 1 toggle (the second stream destroyed and created again), other
    values rejected; a forward in either mode gives the same bits."""
    from gaussiansplattingviewer_amd import _lib
    P, W, H = 30_000, 480, 320
    _, dg, cams = _scene(gpu, P, W, H, 2, seed=17)
    lib = _lib.load_library()
    ctx = _lib.context(0, 0)
    assert lib.gsr_set_option(ctx, _lib.GSR_OPT_SECOND_STREAM, 2) != 0
    assert lib.gsr_set_option(ctx, _lib.GSR_OPT_SECOND_STREAM, -1) != 0
    out = []
    try:
        for v in (0, 1, 0, 1):
            _lib.check(lib.gsr_set_option(ctx, _lib.GSR_OPT_SECOND_STREAM, v), "gsr_set_option")
            r = _render(dg, cams[1], W, H, gpu)
            out.append((r.num_rendered, r.color.clone(), r.radii.clone()))
            torch.cuda.synchronize()
    finally:
        _lib.check(lib.gsr_set_option(ctx, _lib.GSR_OPT_SECOND_STREAM, 1), "gsr_set_option")
    for k, c, rad in out[1:]:
        assert k == out[0][0]
        assert torch.equal(rad, out[0][2])
        assert torch.equal(c.view(torch.int32), out[0][1].view(torch.int32))


def test_one_stream_frames_clustered_scene(gpu):
    """Four one-stream frames in flight on the clustered (c3r-like) scene, whose kept depth keys
    span ~26 bits: those frames take the MSD depth sort (kMsdMaxDOneStream) where a serial
    two-stream forward takes the LSD passes -- every frame must still be bit-identical."""
    from gaussiansplattingviewer_amd.gaussian_data import clustered_scene
    P, W, H, n = 120_000, 640, 480, 9
    g = clustered_scene(P, 5)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    dg = dict(xyz=up(g.xyz), rot=up(g.rot), scale=up(g.scale), opacity=up(g.opacity),
              sh=up(g.sh).reshape(P, -1, 3).contiguous())
    cams = []
    for i in range(n):
        view, proj, campos, tx, ty = cuda_camera_inputs(static_camera(W, H, orbit_eye(i * 11, 1000)))
        cams.append(dict(view=up(view), proj=up(proj), campos=up(campos), tx=tx, ty=ty))
    serial = []
    for cam in cams:
        r = _render(dg, cam, W, H, gpu)
        serial.append((r.num_rendered, r.color.clone(), r.radii.clone()))
    torch.cuda.synchronize()
    pipe = FramePipeline(4, gpu)
    assert not pipe.second_stream
    piped = []
    for cam in cams:
        with pipe.frame() as slot:
            r = _render(dg, cam, W, H, gpu, slot=slot)
            piped.append((r.num_rendered, r.color, r.radii))
    torch.cuda.synchronize()
    FramePipeline(4, gpu, graphs=False, second_stream=True)
    for (k0, c0, r0), (k1, c1, r1) in zip(serial, piped):
        assert k0 == k1
        assert torch.equal(r0, r1)
        assert torch.equal(c0.view(torch.int32), c1.view(torch.int32))


def test_pipeline_close_restores_slot0_options(gpu):
    """FramePipeline changes slot 0's frame-graph and second-stream options (slot 0 is the
    caller's own context) and close() gives the caller back what it had."""
    from gaussiansplattingviewer_amd import _lib
    ctx = _lib.context(gpu.index or 0, 0)
    _lib.set_option(ctx, _lib.GSR_OPT_SECOND_STREAM, 1)
    _lib.set_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS, 2)
    with FramePipeline(4, gpu) as pipe:
        assert not pipe.second_stream
        assert _lib.get_option(ctx, _lib.GSR_OPT_SECOND_STREAM) == 0
        assert _lib.get_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS) == 0
    assert _lib.get_option(ctx, _lib.GSR_OPT_SECOND_STREAM) == 1
    assert _lib.get_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS) == 2
    _lib.set_option(ctx, _lib.GSR_OPT_FRAME_GRAPHS, 0)
    for opt in (_lib.GSR_OPT_BLEND_CULL, _lib.GSR_OPT_BLEND_FAST, _lib.GSR_OPT_TIGHT_BINNING):
        assert _lib.get_option(ctx, opt) == 1
    assert _lib.get_option(ctx, _lib.GSR_OPT_DEPTH_SORT) == -1
    with pytest.raises(RuntimeError, match="unknown option"):
        _lib.get_option(ctx, 10)


def test_threads_and_streams_share_one_context(gpu):
    """Two host threads render through one context (slot 0) at once, each on a stream of its
    own: the context's mutex serialises the calls and a stream switch waits for the previous
    stream's work, so every frame equals its serial render."""
    import threading
    P, W, H, n = 40_000, 480, 320, 6
    _, dg, cams = _scene(gpu, P, W, H, n, seed=23)
    ref = []
    for cam in cams:
        r = _render(dg, cam, W, H, gpu)
        ref.append((r.num_rendered, r.color.clone()))
    torch.cuda.synchronize()
    out = {}
    errors = []

    def worker(t):
        try:
            s = torch.cuda.Stream(gpu)
            with torch.cuda.stream(s):
                for rep in range(4):
                    for i in range(t, n, 2):
                        r = _render(dg, cams[i], W, H, gpu)
                        out[(t, rep, i)] = (r.num_rendered, r.color)
            s.synchronize()
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    assert len(out) == 4 * n
    for (t, rep, i), (k, color) in out.items():
        assert k == ref[i][0]
        assert torch.equal(color.view(torch.int32), ref[i][1].view(torch.int32)), (t, rep, i)


def _bits_equal(a, b):
    assert a.num_rendered == b.num_rendered
    assert torch.equal(a.radii, b.radii)
    assert torch.equal(a.color.view(torch.int32), b.color.view(torch.int32))


def test_empty_frame_state_then_normal_frame(gpu):
    """An empty frame (P = 0) leaves an exported state of its own -- no list entries, all-zero
    ranges and row counts -- and the next frame on that context equals a fresh context's."""
    from gaussiansplattingviewer_amd.rasterizer import binning_state, tile_row_pairs
    used, fresh = 200, 201
    W, H = 64, 48
    view, proj, campos, tx, ty = cuda_camera_inputs(static_camera(W, H))
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    r = rasterize_gaussians_native(
        torch.full((3,), 0.3, device=gpu), torch.zeros((0, 3), device=gpu), None,
        torch.zeros((0, 1), device=gpu), torch.zeros((0, 3), device=gpu),
        torch.zeros((0, 4), device=gpu), 1.0, None, up(view), up(proj), tx, ty, H, W,
        torch.zeros((0, 1, 3), device=gpu), 0, up(campos), False, False, slot=used)
    assert r.num_rendered == 0 and r.radii.shape == (0,)
    assert torch.all(r.color == 0)
    pl, pt, rg = binning_state(0, used)
    assert pl.numel() == 0 and pt.numel() == 0
    assert tuple(rg.shape) == (4 * 3, 2) and not rg.any()
    assert not tile_row_pairs(3, 0, used).any()

    P, W, H = 2_000, 320, 240
    _, dg, cams = _scene(gpu, P, W, H, 1, seed=29)
    a = _render(dg, cams[0], W, H, gpu, slot=used)
    sa = binning_state(0, used)
    b = _render(dg, cams[0], W, H, gpu, slot=fresh)
    sb = binning_state(0, fresh)
    _bits_equal(a, b)
    assert a.num_rendered > 0 and sa[0].numel() > 0
    for x, y in zip(sa, sb):
        assert torch.equal(x, y)


def test_stage_timing_leaves_the_frame_alone(gpu):
    """gsr_set_timing 1 (every stage) and 2 (the blend of every 8th forward) change no output
    bit, with and without frame graphs, and gsr_stage_times reports finite, non-negative means
    with the stages that always run above zero; with no timed forward it is a state error."""
    import ctypes
    from gaussiansplattingviewer_amd import _lib
    from gpu_helpers import set_option
    P, W, H, n = 10_000, 320, 240, 9
    _, dg, cams = _scene(gpu, P, W, H, n, seed=31)
    lib = _lib.load_library()
    names = _lib.stage_names()
    i_pre, i_blend = names.index("preprocess"), names.index("blend")

    def times(ctx):
        buf = (ctypes.c_float * 8)(*([float("nan")] * 8))
        rc = lib.gsr_stage_times(ctx, buf, 8)
        return rc, np.array(buf[:], np.float32)

    for slot, graphs in ((202, 0), (203, 1)):
        set_option(gpu, _lib.GSR_OPT_FRAME_GRAPHS, graphs, slot)
        ctx = _lib.context(0, slot)
        _lib.check(lib.gsr_set_timing(ctx, 0), "gsr_set_timing")
        ref = [_render(dg, cam, W, H, gpu, slot=slot) for cam in cams]
        torch.cuda.synchronize()

        _lib.check(lib.gsr_set_timing(ctx, 1), "gsr_set_timing")
        for cam, want in zip(cams[:3], ref):
            _bits_equal(_render(dg, cam, W, H, gpu, slot=slot), want)
        rc, ms = times(ctx)
        assert rc == 8
        assert np.all(np.isfinite(ms)) and np.all(ms >= 0), ms
        assert ms[i_pre] > 0 and ms[i_blend] > 0, ms

        _lib.check(lib.gsr_set_timing(ctx, 2), "gsr_set_timing")
        for cam, want in zip(cams, ref):  # the 1st and the 9th forward are sampled
            _bits_equal(_render(dg, cam, W, H, gpu, slot=slot), want)
        rc, ms = times(ctx)
        assert rc == 8 and ms[i_blend] > 0, (rc, ms)

        _lib.check(lib.gsr_set_timing(ctx, 0), "gsr_set_timing")
        for cam, want in zip(cams[:2], ref):
            _bits_equal(_render(dg, cam, W, H, gpu, slot=slot), want)
        rc, _ = times(ctx)
        assert rc == -4  # GSR_E_STATE: no timed forward since gsr_set_timing
        if graphs:
            assert _lib.frame_graph_stats(0, slot)["graph_frames"] > 0
