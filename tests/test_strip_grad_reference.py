"""CPU: the premise, the yardstick and the host-side plumbing of the backward on tile row strips
(gsr_backward_strip).  Everything about the reference comes from the C oracle's lists
and the float64 reference alone: the strip reference equals the walk over every tile, the strips'
references add up to the whole frame's, the float32 spread the GPU tolerance of
test_gpu_strip_backward.py is built from is re-measured, and every strip holds the conditions
strip_grad_scenes states.  The entry points validate before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import frame_grad_scenes as fs
import strip_grad_scenes as ss
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    rasterize_gaussians_backward_native)
from gaussiansplattingviewer_amd.strips import reduce_gradients

SUMMED = ("means3D", "means2D", "opacity", "shs", "scales", "rotations", "means2D_px", "conic",
          "rgb", "viewmatrix", "projmatrix", "campos")


def test_strips_are_partitions():
    for name, strips in ss.STRIPS.items():
        _, gy = ss.grid(fs.get(name))
        assert strips[0][0] == 0 and strips[-1][1] == gy
        assert all(a[1] == b[0] for a, b in zip(strips, strips[1:]))
        assert all(b < e for b, e in strips)
    sc = fs.get("frame")
    assert ss.pixel_rows(sc, (8, 9)) == (128, 136)  # rows = 8, not 16 (e - b)
    assert ss.local_dL(sc, (8, 9))[0].shape == (3, 8, 200)
    assert ss.local_dL(sc, (8, 9))[1].shape == (3, 8, 200)
    tall = fs.get("tall")
    assert ss.STRIPS["tall"][1][1] - ss.STRIPS["tall"][1][0] == 256 and ss.grid(tall)[1] == 257


def test_strip_reference_equals_the_walk_over_every_tile():
    """wall, float64: a pixel with zero image gradients adds exactly nothing, so walking the
    strip's tiles alone changes no gradient beyond the order of a few hundred float64 adds."""
    sc = fs.get("wall")
    for strip in ss.STRIPS["wall"]:
        a = ss.reference(sc, strip, "colour")
        b = ss.reference(sc, strip, "colour", every_tile=True)
        for k in SUMMED:
            if k in a:
                m = np.abs(b[k]).max()
                assert m > 0 and np.abs(a[k] - b[k]).max() <= 1e-12 * m, (strip, k)


@pytest.mark.parametrize("name,kind", [(n, k) for n in ss.STRIPS for k in ss.KINDS[n]])
def test_strips_add_up_to_the_whole_frame(name, kind):
    """Linearity, a property of the reference: in float64 the strips' references add up to
    fs.reference to 1e-12 of the largest entry (round-off of a few hundred adds)."""
    sc = fs.get(name)
    whole = fs.reference(sc, kind)
    parts = [ss.reference(sc, strip, kind) for strip in ss.STRIPS[name]]
    seen = 0
    for k in SUMMED:
        if k not in whole:
            continue
        total = sum(p[k] for p in parts)
        m = np.abs(whole[k]).max()
        assert m > 0 and np.abs(total - whole[k]).max() <= 1e-12 * m, (k, np.abs(total - whole[k]).max() / m)
        seen += 1
    assert seen >= 6


@pytest.mark.parametrize("name,strip", ss.CASES)
def test_strip_conditions(name, strip):
    sc = fs.get(name)
    y0, y1 = ss.pixel_rows(sc, strip)
    m = fs.mask(sc)[y0:y1]
    ids, n = fs.quadrants(sc)
    ids = ids[y0:y1]
    inside = np.bincount(ids.ravel(), minlength=n)
    hit = np.bincount(ids.ravel(), m.ravel().astype(np.float64), n)
    assert m.mean() <= fs.MASK_CAP
    assert ((inside - hit) >= fs.QUADRANT_KEEP * inside).all()
    ins, clip, none = ss.classes(sc, strip)
    print(f"{name} {strip}: masked {m.mean():.4f}; inside {ins.sum()}, clipped {clip.sum()}, "
          f"without a tile {none.sum()}")
    assert ins.sum() + clip.sum() + none.sum() == len(ins) and not (ins & clip).any()
    assert clip.sum() >= 1
    if name != "wall":  # (wall: over the partition, below; strip_grad_scenes says why)
        assert ins.sum() >= 1 and none.sum() >= 1
    # the strip's image gradients are the masked ones inside its rows, zero outside
    dL, dLp = ss.full_dL(sc, strip)
    ref = fs.masked(sc)
    for a, b in zip((dL, dLp), ref):
        assert (a[:, y0:y1] == b[:, y0:y1]).all() and (a[:, :y0] == 0).all() and (a[:, y1:] == 0).all()


def test_wall_classes_over_the_partition():
    sc = fs.get("wall")
    got = [ss.classes(sc, strip) for strip in ss.STRIPS["wall"]]
    assert any(c[0].sum() >= 1 for c in got) and any(c[2].sum() >= 1 for c in got)
    assert all(c[1].sum() >= 400 for c in got)  # Gaussians straddling the cut


def test_frame_big_gaussians_are_clipped_by_every_cut():
    sc = fs.get("frame")
    for strip in ss.STRIPS["frame"]:
        assert ss.classes(sc, strip)[1][sc["special"]["big"]].all(), strip


@pytest.mark.parametrize("name,strip,kind", sorted(ss.F32_SPREAD))
def test_float32_spread_constants(name, strip, kind):
    """ss.F32_SPREAD is what a float32 evaluation of the strip reference gives here, each constant
    within a factor 2 either way (frame_grad_scenes' rule)."""
    table = ss.F32_SPREAD[(name, strip, kind)]
    seen = ss.spread(fs.get(name), strip, kind, [k for k in table if k != "colors"])
    print({k: f"{v:.3e}" for k, v in seen.items()})
    assert set(seen) == set(table) - {"colors"}
    assert set(table) - {"colors"} == set(fs.F32_SPREAD[(name, kind)]) - {"colors"}
    for k, f in seen.items():
        assert 0.5 * f <= table[k] <= 2.0 * f, (k, f, table[k])
    assert ss.bound(name, strip, kind, "means3D") == 8.0 * table["means3D"]


def test_every_case_has_its_constants():
    assert set(ss.F32_SPREAD) == {(n, s, k) for n, s in ss.CASES for k in ss.KINDS[n]}


# ---- the host side ----------------------------------------------------------------------------------
def test_strip_host_abi():
    """gsr_backward_strip is exported, additive to ABI 4, and validates before any device work."""
    lib = _lib.load_library()
    assert lib.gsr_abi_version() == _lib.ABI_VERSION == 4
    assert "gsr_backward_strip" in _lib.EXPORTED_SYMBOLS
    bw = _lib.backward_strip_fn(lib)
    assert bw is lib.gsr_backward_strip and bw.restype is ctypes.c_int and len(bw.argtypes) == 10

    class Old:  # (a build of ABI 4 from before the entry)
        pass
    with pytest.raises(RuntimeError, match="no gsr_backward_strip"):
        _lib.backward_strip_fn(Old())
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)  # never dereferenced
    g, st = _lib.GsrGaussians(P=4), _lib.GsrRasterSettings(image_width=40, image_height=40)
    inp, gr_ = _lib.GsrBackwardInputs(), _lib.GsrGradients()
    ref = ctypes.byref
    # a NULL argument, with and without a strip
    for rb, re in ((0, 0), (0, 1)):
        st.tile_row_begin, st.tile_row_end = rb, re
        for args in ((None, ref(g), ref(st), ref(inp), ref(gr_)), (ctx, None, ref(st), ref(inp), ref(gr_)),
                     (ctx, ref(g), None, ref(inp), ref(gr_)), (ctx, ref(g), ref(st), None, ref(gr_)),
                     (ctx, ref(g), ref(st), ref(inp), None)):
            assert bw(*args[:4], None, None, None, None, args[4], None) == -1
            assert b"NULL argument" in lib.gsr_last_error()
    # a bad strip (the frame has 3 tile rows), a bad mode, a bad filter: before the context is touched
    for rb, re in ((-1, 2), (0, 4), (2, 2), (2, 1), (3, 0)):
        st.tile_row_begin, st.tile_row_end = rb, re
        for o in (None, ref(_lib.GsrBackwardOrder(deterministic=1))):
            assert bw(ctx, ref(g), ref(st), ref(inp), None, None, None, o, ref(gr_), None) == -1
            assert b"gsr_backward_strip: bad tile row strip" in lib.gsr_last_error()
    st.tile_row_begin, st.tile_row_end = 1, 3
    o = _lib.GsrBackwardOrder(deterministic=2)
    assert bw(ctx, ref(g), ref(st), ref(inp), None, None, None, ref(o), ref(gr_), None) == -1
    assert b"gsr_backward_strip: deterministic must be 0 or 1" in lib.gsr_last_error()
    bad_filter = _lib.GsrFilterSettings(antialiasing=2)
    assert bw(ctx, ref(g), ref(st), ref(inp), None, None, ref(bad_filter), None, ref(gr_), None) == -1
    assert b"antialiasing must be 0 or 1" in lib.gsr_last_error()
    # (P > 0 without an image gradient: refused before the context is touched, as a whole frame)
    for o in (None, ref(_lib.GsrBackwardOrder(deterministic=1))):
        assert bw(ctx, ref(g), ref(st), ref(inp), None, None, None, o, ref(gr_), None) == -1
        assert b"gsr_backward_strip: dL_dcolor is required" in lib.gsr_last_error()
    # without a strip it is gsr_backward_ordered, by its own messages
    st.tile_row_begin = st.tile_row_end = 0
    assert bw(ctx, ref(g), ref(st), ref(inp), None, None, None, o, ref(gr_), None) == -1
    assert b"dL_dcolor is required" in lib.gsr_last_error()
    assert b"gsr_backward_strip" not in lib.gsr_last_error()
    # every other backward entry still refuses a strip
    st.tile_row_begin, st.tile_row_end = 1, 3
    assert lib.gsr_backward_ordered(ctx, ref(g), ref(st), ref(inp), None, None, None, None,
                                    ref(gr_), None) == -1
    assert b"whole frames only" in lib.gsr_last_error()


def _native_args(dL):
    P = 5
    return (torch.zeros(3), torch.zeros(P, 3), None, torch.ones(P, 1), torch.ones(P, 3),
            torch.ones(P, 4), 1.0, None, torch.eye(4), torch.eye(4), 0.5, 0.5, dL,
            torch.zeros(P, 16, 3), 3, torch.zeros(3))


def test_native_backward_validates_the_strip_on_the_host():
    """tile_rows needs image_height; the image and plane gradients must be the strip's: raised
    before any device is asked for (the inputs are host tensors)."""
    with pytest.raises(RuntimeError, match="tile_rows needs image_height"):
        rasterize_gaussians_backward_native(*_native_args(torch.zeros(3, 16, 40)), tile_rows=(0, 1))
    with pytest.raises(RuntimeError, match="image_height belongs to tile_rows"):
        rasterize_gaussians_backward_native(*_native_args(torch.zeros(3, 40, 40)), image_height=40)
    # a frame 40 px high: tile rows (2, 3) are its last 8 rows
    with pytest.raises(RuntimeError, match="must have 8 rows, got 16"):
        rasterize_gaussians_backward_native(*_native_args(torch.zeros(3, 16, 40)), tile_rows=(2, 3),
                                            image_height=40)
    with pytest.raises(RuntimeError, match="must have 32 rows, got 40"):
        rasterize_gaussians_backward_native(*_native_args(torch.zeros(3, 40, 40)), tile_rows=(0, 2),
                                            image_height=40)
    for bad in ((0, 4), (2, 2), (-1, 1)):
        with pytest.raises(RuntimeError, match="outside"):
            rasterize_gaussians_backward_native(*_native_args(torch.zeros(3, 16, 40)),
                                                tile_rows=bad, image_height=40)
    with pytest.raises(RuntimeError, match=r"dL_dfinal_T must have dimensions \(H, W\) = \(8, 40\)"):
        rasterize_gaussians_backward_native(*_native_args(torch.zeros(3, 8, 40)), tile_rows=(2, 3),
                                            image_height=40, dL_dfinal_T=torch.zeros(40, 40))
    # the right shapes pass the checks and reach the device request
    with pytest.raises(RuntimeError, match="device"):
        rasterize_gaussians_backward_native(*_native_args(torch.zeros(3, 8, 40)), tile_rows=(2, 3),
                                            image_height=40)


def _settings(**kw):
    return GaussianRasterizationSettings(40, 40, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4),
                                         torch.eye(4), 3, torch.zeros(3), False, False, **kw)


def test_settings_carry_tile_rows():
    rs = _settings()
    assert rs.tile_rows is None and len(rs) == 13 and len(rs._fields) == 13
    rs = _settings(tile_rows=[1, 3], deterministic=True, antialiasing=True)
    assert rs.tile_rows == (1, 3) and len(rs) == 13 and rs.deterministic and rs.antialiasing
    r2 = rs._replace(debug=True)
    assert r2.tile_rows == (1, 3) and r2.debug and r2.deterministic is True
    assert rs._replace(tile_rows=None).tile_rows is None
    assert rs._replace(tile_rows=(0, 1)).tile_rows == (0, 1)
    with pytest.raises(TypeError):
        GaussianRasterizationSettings(40, 40, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4),
                                      torch.eye(4), 3, torch.zeros(3), False, False, 0, False,
                                      (0, 1))  # keyword only


def test_extension_entries_take_the_strip():
    from gaussiansplattingviewer_amd import _native
    fwd = _native.rasterize_gaussians_ext.__doc__.splitlines()[0]
    assert fwd.count(":") == 24 and fwd.count(" = 0") == 2
    assert fwd.index("tile_row_begin") < fwd.index(" = 0") < fwd.index("tile_row_end")
    assert fwd.index("antialiasing") < fwd.index("tile_row_begin")
    bwd = _native.rasterize_gaussians_backward_strip_ext.__doc__.splitlines()[0]
    assert bwd.count(":") == 26, bwd
    # upstream's two entries are untouched
    assert _native.rasterize_gaussians.__doc__.splitlines()[0].count(":") == 19
    assert _native.rasterize_gaussians_backward.__doc__.splitlines()[0].count(":") == 22


def test_reduce_gradients_is_a_noop_at_world_one(tmp_path):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0,
                            world_size=1)
    try:
        t = torch.arange(6, dtype=torch.float32)
        reduce_gradients([t, None])
        assert torch.equal(t, torch.arange(6, dtype=torch.float32))
    finally:
        dist.destroy_process_group()
