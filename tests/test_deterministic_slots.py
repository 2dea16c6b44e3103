"""CPU: the premise and the plumbing of the deterministic backward (gsr_backward_ordered,
DESIGN.md 3k).

The mode gives every (Gaussian, tile) pair of upstream's lists an address that needs no search,

    pair(id, tx, ty) = slab[id] + (ty - row0) * w + (tx - x0),   slot = pair * 4 + quadrant,

with (x0, row0, w, rows) the Gaussian's tile rect and slab the exclusive scan of w * rows in id
order.  Restated here in Python from the C oracle's float32 means2D and radii (upstream's getRect)
and checked against the oracle's lists on S1-S4 (grad_scenes) and frame, wall, wide, tall
(frame_grad_scenes): over all list entries pair is a bijection onto [0, K); every listed tile lies
inside its Gaussian's rect; a Gaussian with radius 0 owns no slot.

Then the setting (GaussianRasterizationSettings.deterministic), the routing of the three Functions
with `_C` replaced by fakes, and the argument checks of the C entry that return before any device
work."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import frame_grad_scenes as fs
import grad_scenes
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer,
                                                    rasterize_gaussians_backward_native)

F32 = np.float32
SCENES = [("toy", n) for n in grad_scenes.NAMES] + [("frame", n) for n in fs.NAMES]


def _scene(kind, name):
    return grad_scenes.get(name) if kind == "toy" else fs.get(name)


def rects(means2D, radii, W, H):
    """(x0, y0, w, rows) per Gaussian, int64: upstream's getRect in float32 (the quotient by the
    tile size truncated towards zero, clamped to the grid); w = rows = 0 for radius 0."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    px, py = means2D[:, 0].astype(F32), means2D[:, 1].astype(F32)
    r = radii.astype(F32)
    lo = lambda p, g: np.clip(np.trunc((p - r) / F32(16)).astype(np.int64), 0, g)  # noqa: E731
    hi = lambda p, g: np.clip(np.trunc((p + r + F32(15)) / F32(16)).astype(np.int64), 0, g)  # noqa: E731
    x0, x1, y0, y1 = lo(px, gx), hi(px, gx), lo(py, gy), hi(py, gy)
    live = (radii > 0) & (x1 > x0) & (y1 > y0)
    w, rows = np.where(live, x1 - x0, 0), np.where(live, y1 - y0, 0)
    return x0, y0, w, rows


def slab_of(w, rows):
    """The exclusive scan of w * rows in id order, and its total."""
    n = (w * rows).astype(np.int64)
    return np.concatenate([[0], np.cumsum(n)[:-1]]), int(n.sum())


def pairs_of(orc, W, H):
    """pair of every list entry in list order, with the entries' ids, tile coordinates and
    rects."""
    gx = (W + 15) // 16
    x0, y0, w, rows = rects(orc["means2D"], orc["radii"], W, H)
    slab, total = slab_of(w, rows)
    ranges = np.asarray(orc["ranges"]).reshape(-1, 2).astype(np.int64)
    ids = np.asarray(orc["point_list"]).astype(np.int64)
    tile = np.repeat(np.arange(len(ranges)), ranges[:, 1] - ranges[:, 0])
    order = np.concatenate([np.arange(a, b) for a, b in ranges]) if len(ranges) else np.zeros(0, int)
    assert len(order) == len(ids) and (np.sort(order) == np.arange(len(ids))).all()
    tile_of = np.empty(len(ids), np.int64)
    tile_of[order] = tile
    tx, ty = tile_of % gx, tile_of // gx
    pair = slab[ids] + (ty - y0[ids]) * w[ids] + (tx - x0[ids])
    return dict(pair=pair, ids=ids, tx=tx, ty=ty, x0=x0, y0=y0, w=w, rows=rows, slab=slab,
                total=total)


@pytest.mark.parametrize("kind,name", SCENES, ids=[n for _, n in SCENES])
def test_pair_is_a_bijection_onto_the_list(kind, name):
    sc = _scene(kind, name)
    orc = fs.oracle_of(sc)
    p = pairs_of(orc, sc["W"], sc["H"])
    K = int(orc["num_rendered"])
    ids = p["ids"]
    assert K == len(ids) == p["total"] > 0
    # every listed tile lies inside its Gaussian's rect
    assert ((p["tx"] >= p["x0"][ids]) & (p["tx"] < p["x0"][ids] + p["w"][ids])).all()
    assert ((p["ty"] >= p["y0"][ids]) & (p["ty"] < p["y0"][ids] + p["rows"][ids])).all()
    # ... and pair maps the entries one to one onto [0, K)
    assert (np.sort(p["pair"]) == np.arange(K)).all()
    # a Gaussian's pairs are its own segment of [0, K), in id order
    n = p["w"] * p["rows"]
    assert ((p["pair"] >= p["slab"][ids]) & (p["pair"] < p["slab"][ids] + n[ids])).all()
    # radius 0: no slot
    culled = np.asarray(orc["radii"]) == 0
    assert (n[culled] == 0).all() and not np.isin(ids, np.flatnonzero(culled)).any()
    assert (n == np.bincount(ids, minlength=len(n))).all()
    assert 4 * K < 2 ** 32  # the slots of these scenes fit the 32-bit index by far


def test_scenes_cover_the_cases():
    """frame's four large Gaussians own all 117 tiles; S4 and wall hold Gaussians without a slot
    (culled) and wall Gaussians with slots nothing is stored to."""
    frame = fs.get("frame")
    p = pairs_of(fs.oracle_of(frame), frame["W"], frame["H"])
    assert ((p["w"] * p["rows"])[frame["special"]["big"]] == 117).all()
    edges = grad_scenes.get("edges")
    assert (np.asarray(fs.oracle_of(edges)["radii"])[edges["special"]["behind"]] == 0).all()
    wide = fs.get("wide")
    assert (wide["W"] + 15) // 16 == 257


# ---- the setting ------------------------------------------------------------------------------
def _settings(**kw):
    eye = torch.eye(4)
    return GaussianRasterizationSettings(4, 6, 0.5, 0.4, torch.zeros(3), 1.0, eye, eye, 3,
                                         torch.zeros(3), False, False, **kw)


def test_setting_is_keyword_only_and_an_attribute():
    rs = _settings()
    assert rs.deterministic is None and len(rs) == 13 == len(GaussianRasterizationSettings._fields)
    assert "deterministic" not in GaussianRasterizationSettings._fields
    params = list(inspect.signature(GaussianRasterizationSettings.__new__).parameters)
    assert params[-2:] == ["depth_maps", "kwargs"]
    for v in (True, False, None):
        rs = _settings(deterministic=v)
        assert rs.deterministic is v and len(rs) == 13
        assert rs._replace(debug=True).deterministic is v          # carried
        assert rs._replace(antialiasing=True).deterministic is v
    rs = _settings(deterministic=True, antialiasing=True, depth_maps=True)
    assert (rs.deterministic, rs.antialiasing, rs.depth_maps) == (True, True, True)
    assert rs._replace(deterministic=None).deterministic is None
    assert rs._replace(deterministic=0).deterministic is False
    assert rs._replace(deterministic=False).antialiasing is True
    assert _settings(deterministic=1).deterministic is True
    with pytest.raises(TypeError):  # not positional: 13 fields, then depth_maps
        GaussianRasterizationSettings(4, 6, 0.5, 0.4, torch.zeros(3), 1.0, torch.eye(4),
                                      torch.eye(4), 3, torch.zeros(3), False, False, 0, False, True)
    p = inspect.signature(rasterize_gaussians_backward_native).parameters["deterministic"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


# ---- the routing ----------------------------------------------------------------------------------
def _fake_C(monkeypatch, seen):
    """`_C`'s four entries replaced by fakes that record their arguments (test_abi_host._fake_C's
    style; the general backward takes 22 or 23 arguments here)."""
    from gaussiansplattingviewer_amd import _C

    def forward(name):
        def fake(*args):
            seen.setdefault(name, []).append(args)
            P, (H, W) = args[1].shape[0], args[12:14]
            planes = len(args) == 22 and args[20]
            maps = [torch.full((H, W), float(i)) if planes else torch.empty(0) for i in range(3)]
            return (7, torch.zeros(3, H, W), torch.ones(P, dtype=torch.int32), *maps)
        return fake

    def backward(name, counts, sh_at):
        def fake(*args):
            assert len(args) in counts, (name, len(args))
            seen.setdefault(name, []).append(args)
            P, M = args[1].shape[0], args[sh_at].shape[1]
            g = tuple(torch.full(s, float(i)) for i, s in enumerate(
                ((P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, M, 3), (P, 3), (P, 4))))
            if name.endswith("_ext"):
                g += tuple(torch.full(s, 9.0) if args[20] else torch.empty(0)
                           for s in ((4, 4), (4, 4), (3,)))
            return g
        return fake

    monkeypatch.setattr(_C, "rasterize_gaussians", forward("rasterize_gaussians"))
    monkeypatch.setattr(_C, "rasterize_gaussians_ext", forward("rasterize_gaussians_ext"))
    monkeypatch.setattr(_C, "rasterize_gaussians_backward",
                        backward("rasterize_gaussians_backward", (22,), 13))
    monkeypatch.setattr(_C, "rasterize_gaussians_backward_ext",
                        backward("rasterize_gaussians_backward_ext", (22, 23), 12))


def _one_backward(seen, deterministic, depth_maps=False, antialiasing=False, camera=False):
    P = 5
    xyz, op = torch.zeros(P, 3, requires_grad=True), torch.ones(P, 1, requires_grad=True)
    sc, rot = torch.ones(P, 3, requires_grad=True), torch.ones(P, 4, requires_grad=True)
    sh = torch.zeros(P, 16, 3, requires_grad=True)
    view = torch.eye(4, requires_grad=camera)
    rs = GaussianRasterizationSettings(4, 6, 0.5, 0.4, torch.zeros(3), 1.0, view, torch.eye(4), 3,
                                       torch.zeros(3), False, False, depth_maps=depth_maps,
                                       antialiasing=antialiasing, deterministic=deterministic)
    seen.clear()
    out = GaussianRasterizer(rs)(means3D=xyz, means2D=None, opacities=op, shs=sh,
                                 colors_precomp=None, scales=sc, rotations=rot, cov3D_precomp=None)
    (out[0].sum() + (out[2].sum() if depth_maps else 0.0)).backward()
    assert (xyz.grad == 3).all() and (sh.grad == 5).all()
    if camera:
        assert (view.grad == 9).all()


@pytest.mark.parametrize("depth_maps,antialiasing,camera", [
    (False, False, False), (True, False, False), (False, True, False), (False, False, True),
    (True, True, True)])
def test_functions_pass_the_mode_only_when_it_is_on(depth_maps, antialiasing, camera, monkeypatch):
    """All three Functions: without the mode today's calls (upstream's backward for the plain
    frame, else 22 arguments ending (camera, antialiasing)); with it the general entry with a
    23rd argument, True -- for the plain frame too."""
    seen = {}
    _fake_C(monkeypatch, seen)
    mode = (depth_maps, antialiasing, camera)
    for det in (False, None):  # (the global switch is off)
        assert not torch.are_deterministic_algorithms_enabled()
        _one_backward(seen, det, *mode)
        if any(mode):
            (b,) = seen["rasterize_gaussians_backward_ext"]
            assert len(b) == 22 and b[20:] == (camera, antialiasing)
            assert "rasterize_gaussians_backward" not in seen
        else:
            (b,) = seen["rasterize_gaussians_backward"]
            assert len(b) == 22 and "rasterize_gaussians_backward_ext" not in seen
    _one_backward(seen, True, *mode)
    assert "rasterize_gaussians_backward" not in seen
    (b,) = seen["rasterize_gaussians_backward_ext"]
    assert len(b) == 23 and b[20:] == (camera, antialiasing, True)
    assert tuple(b[16].shape) == (3, 4, 6) and b[15] is False
    assert tuple(b[17].shape) == ((4, 6) if depth_maps else (0,))


def test_none_follows_the_torch_switch_at_backward_time(monkeypatch):
    seen = {}
    _fake_C(monkeypatch, seen)
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        _one_backward(seen, None)
        (b,) = seen["rasterize_gaussians_backward_ext"]
        assert len(b) == 23 and b[22] is True
        _one_backward(seen, False)  # False forces the default path under the switch
        assert "rasterize_gaussians_backward_ext" not in seen
        assert len(seen["rasterize_gaussians_backward"][0]) == 22
        # read when the backward runs, not when the frame was rendered
        torch.use_deterministic_algorithms(False)
        P = 5
        xyz = torch.zeros(P, 3, requires_grad=True)
        rs = _settings()
        seen.clear()
        color, _ = GaussianRasterizer(rs)(means3D=xyz, means2D=None, opacities=torch.ones(P, 1),
                                          shs=torch.zeros(P, 16, 3), colors_precomp=None,
                                          scales=torch.ones(P, 3), rotations=torch.ones(P, 4),
                                          cov3D_precomp=None)
        torch.use_deterministic_algorithms(True)
        color.sum().backward()
        assert len(seen["rasterize_gaussians_backward_ext"][0]) == 23
    finally:
        torch.use_deterministic_algorithms(was)
    assert torch.are_deterministic_algorithms_enabled() == was


def test_extension_signature_has_the_trailing_default():
    from gaussiansplattingviewer_amd import _native
    sig = _native.rasterize_gaussians_backward_ext.__doc__.splitlines()[0]
    assert sig.count(":") == 23 and "deterministic: bool = False" in sig, sig
    assert sig.index("antialiasing") < sig.index("deterministic")


# ---- the C entry ----------------------------------------------------------------------------------
def test_ordered_host_abi():
    """gsr_backward_ordered is exported, additive to ABI 4, and validates before any device work:
    a mode other than 0 or 1 is GSR_E_INVALID whatever else is passed; NULL and 0 take
    gsr_backward_filtered's checks, 1 the same ones; a strip is GSR_E_INVALID in every mode."""
    lib = _lib.load_library()
    assert lib.gsr_abi_version() == _lib.ABI_VERSION == 4
    assert "gsr_backward_ordered" in _lib.EXPORTED_SYMBOLS
    bw = _lib.backward_ordered_fn(lib)
    assert bw is lib.gsr_backward_ordered and bw.restype is ctypes.c_int
    assert len(bw.argtypes) == 10 and ctypes.sizeof(_lib.GsrBackwardOrder) == 4

    class Old:  # (a build of ABI 4 from before the entry)
        pass
    with pytest.raises(RuntimeError, match="no gsr_backward_ordered"):
        _lib.backward_ordered_fn(Old())
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)  # never dereferenced
    g, st = _lib.GsrGaussians(P=4), _lib.GsrRasterSettings(image_width=8, image_height=8)
    inp, gr_ = _lib.GsrBackwardInputs(), _lib.GsrGradients()
    ref = ctypes.byref
    for v in (2, -1, 255):
        o = _lib.GsrBackwardOrder(deterministic=v)
        assert bw(ctx, ref(g), ref(st), ref(inp), None, None, None, ref(o), ref(gr_), None) == -1
        assert b"deterministic must be 0 or 1" in lib.gsr_last_error()
        assert bw(None, None, None, None, None, None, None, ref(o), None, None) == -1
        assert b"deterministic must be 0 or 1" in lib.gsr_last_error()
    bad_filter = _lib.GsrFilterSettings(antialiasing=2)
    for o in (None, ref(_lib.GsrBackwardOrder(deterministic=0)),
              ref(_lib.GsrBackwardOrder(deterministic=1))):
        assert bw(None, ref(g), ref(st), ref(inp), None, None, None, o, ref(gr_), None) == -1
        assert bw(ctx, ref(g), ref(st), None, None, None, None, o, ref(gr_), None) == -1
        assert bw(ctx, ref(g), ref(st), ref(inp), None, None, None, o, None, None) == -1
        assert bw(ctx, ref(g), ref(st), ref(inp), None, None, ref(bad_filter), o, ref(gr_),
                  None) == -1
        assert b"antialiasing must be 0 or 1" in lib.gsr_last_error()
        st.tile_row_begin, st.tile_row_end = 0, 1
        assert bw(ctx, ref(g), ref(st), ref(inp), None, None, None, o, ref(gr_), None) == -1
        assert b"whole frames only" in lib.gsr_last_error()
        st.tile_row_end = 0
        # (P > 0 without an image gradient: refused before the context is touched)
        assert bw(ctx, ref(g), ref(st), ref(inp), None, None, None, o, ref(gr_), None) == -1
        assert b"dL_dcolor is required" in lib.gsr_last_error()
