"""GPU: the deterministic backward (gsr_backward_ordered with deterministic = 1):
every gradient of a call, the camera's three included, has the same bits on every call with the
same inputs -- whichever context or option set runs it, whatever ran before -- and the numbers are
the default backward's up to the rounding of the sums over pixels.

   1 reproducible: frame, wall, wide, tall under a dense, unmasked gradient on the image and the
     three planes, camera and antialiasing on: three calls on one context, one on a fresh one, one
     after another scene's forward and backward; every tensor bit for bit
   2 frame: the same bits under every depth sort form, without the second stream, without the
     blend cull
   3 every degree-3 SH layout with a gradient on every pixel: the base layout's bits, exact zeros
     above the active degree and for culled Gaussians
   4 where the atomic path is exact too -- the image gradient in the eight parts of dL_masks (at
     most two addends per row) or in one quadrant (one addend) -- the default call's bits in every
     tensor, and exact zeros outside the one tile's list
   5 accuracy against float64 autograd within the project's own bounds, unchanged: S1-S4 (8 x f
     of grad_reference / aa_reference) and frame, wall, wide, tall (frame_grad_scenes.bound under
     the masked gradients), colour alone and colour + planes + camera + antialiasing
   6 exact zeros: wall's uncomposited Gaussians, every culled Gaussian
   7 one context through frame, S1, frame with the camera, wide, S1: each result a fresh context's
     bits (a stale or unzeroed mark fails here)
   8 every entry: ctypes, `_C.rasterize_gaussians_backward_ext`, GaussianRasterizer with
     deterministic=True and with None under torch.use_deterministic_algorithms(True)
   9 errors: deterministic = 2 and a strip are GSR_E_INVALID with nothing written; P = 0 gives zero
     camera sums
  10 off means untouched: a NULL order and deterministic = 0 are gsr_backward_filtered
"""
import ctypes

import numpy as np
import pytest
import torch

import aa_reference as ar
import aa_scenes
import frame_grad_scenes as fs
import grad_scenes
import plane_grad_reference as pg
import sh_layout_scenes as L
from gaussiansplattingviewer_amd import _C, _lib
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer,
                                                    rasterize_gaussians_backward_native)
from gpu_helpers import run_hip, set_option, to_dev
from test_gpu_antialiasing import _assert_close as _aa_assert_close
from test_gpu_antialiasing import _reference as _aa_reference
from test_gpu_backward import END_TO_END, _assert_end_to_end, _inputs
from test_gpu_backward import _reference as _toy_reference
from test_gpu_backward_frames import CAMERA, _all_close, _fwd, _is_zero
from test_gpu_sh_layouts import _sh_dev

pytestmark = pytest.mark.gpu

CAMERA_NAMES = tuple(n for n, _ in CAMERA)
# (context slots of this file alone; test_gpu_backward_frames.py hands out 400 upwards)
OPTION_SLOT = 500
_next_slot = [500]
_dense = {}  # scene -> the dense call of check 1 on slot 0 (check 2 compares with it)


def _new_slot():
    _next_slot[0] += 1
    return _next_slot[0]


def _call(sc, gpu, dL, dLp=None, camera=False, aa=False, det=True, slot=0, conic=True, sh=None,
          colors=None):
    """One native backward as float32 numpy arrays by their gsr_gradients names; with dLp also
    dL_ddepths."""
    s, d = sc["s"], _inputs(sc if colors is None else dict(sc, colors=colors), gpu)
    kw = {}
    if dLp is not None:
        kw = {f"dL_d{n}": to_dev(dLp[i], gpu) for i, n in enumerate(pg.PLANES)}
        kw["depths"] = True
    g = rasterize_gaussians_backward_native(
        to_dev(s["bg"], gpu), d["means3D"], d["colors_precomp"], d["opacities"], d["scales"],
        d["rotations"], s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], to_dev(dL, gpu),
        d["shs"] if sh is None else sh, s["sh_degree"] if colors is None else 0,
        to_dev(s["campos"], gpu), conic=conic, camera=camera, antialiasing=aa, slot=slot,
        deterministic=det, **kw)
    return {k: v.cpu().numpy() for k, v in g.items()}


def _f64(got):
    out = {k: v.astype(np.float64) for k, v in got.items()}
    if "dL_dcampos" in out:
        out["dL_dcampos"] = out["dL_dcampos"].reshape(-1)[:3]
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, ref, what, sh_cols=None):
    assert set(got) == set(ref), what
    for k, v in got.items():
        w = ref[k]
        if k == "dL_dsh" and sh_cols is not None:
            v, w = v[:, :sh_cols], w[:, :sh_cols]
        bad = _bits(v) != _bits(w)
        rows = np.flatnonzero(bad.reshape(len(bad), -1).any(axis=1))
        assert not bad.any(), f"{what}: {k} differs in {bad.sum()} words, rows {rows[:8]}"


def _dense_call(name, gpu, slot=0):
    """Check 1's call: the scene's unmasked dL and dLp, camera and antialiasing on."""
    sc = fs.get(name)
    return _call(sc, gpu, sc["dL"], sc["dLp"], camera=True, aa=True, slot=slot)


# ---- 1 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fs.NAMES)
def test_reproducible(name, gpu):
    first = _dense[name] = _dense_call(name, gpu)
    want = {"dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dcolors", "dL_dconic", "dL_dsh",
            "dL_dscales", "dL_drotations", "dL_ddepths", "dL_dcov3D", *CAMERA_NAMES}
    assert set(first) == want
    for k, v in first.items():
        assert np.isfinite(v).all(), k
        assert np.abs(v).max() > 0 or k == "dL_dcov3D", k  # (scales and rotations: no cov3D)
    for i in (2, 3):
        _same_bits(_dense_call(name, gpu), first, f"{name}: call {i} on one context")
    _same_bits(_dense_call(name, gpu, _new_slot()), first, f"{name}: a fresh context")
    # another scene's forward and backward (both modes) on the same context in between
    other = grad_scenes.get("long_lists") if name != "wall" else fs.get("wide")
    run_hip(other["s"], gpu, colors_precomp=other["colors"], cov3D_precomp=other["cov6"])
    _call(other, gpu, other["dL"], det=False)
    _call(other, gpu, other["dL"])
    _same_bits(_dense_call(name, gpu), first, f"{name}: after another scene")


# ---- 2 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,value", [(_lib.GSR_OPT_DEPTH_SORT, v) for v in (0, 1, 2, 3)] +
                         [(_lib.GSR_OPT_SECOND_STREAM, 0), (_lib.GSR_OPT_BLEND_CULL, 0)],
                         ids=["depth_sort_0", "depth_sort_1", "depth_sort_2", "depth_sort_3",
                              "second_stream_0", "blend_cull_0"])
def test_bits_across_options(opt, value, gpu):
    """frame's dense call under an option: the bits of the default options (a splat the blend
    cull drops has weight exactly 0, so without the cull it is staged, composites nowhere, and
    stores nothing)."""
    if "frame" not in _dense:
        _dense["frame"] = _dense_call("frame", gpu)
    ctx = _lib.context(gpu.index or 0, OPTION_SLOT)
    before = _lib.get_option(ctx, opt)
    set_option(gpu, opt, value, OPTION_SLOT)
    try:
        got = _dense_call("frame", gpu, OPTION_SLOT)
        assert _lib.get_option(ctx, opt) == value
    finally:
        set_option(gpu, opt, before, OPTION_SLOT)
    _same_bits(got, _dense["frame"], f"frame, option {opt} = {value}")


# ---- 3 --------------------------------------------------------------------------------------------
def _layout_call(sc, gpu, mode, det=True, part=None):
    mask = 1.0 if part is None else L.dL_masks()[part]
    rng = np.random.default_rng(77)
    dLp = None
    if mode == "all":
        dLp = [np.ascontiguousarray(rng.standard_normal((L.H, L.W)), np.float32) * mask
               for _ in range(3)]
    return _call(sc, gpu, sc["dL"] * mask, dLp, camera=mode == "all", aa=mode == "all", det=det,
                 sh=_sh_dev(sc, gpu))


@pytest.mark.parametrize("mode", ("plain", "all"))
def test_sh_layouts_with_a_gradient_on_every_pixel(mode, gpu):
    base = L.get("deg3")
    ref = _layout_call(base, gpu, mode)
    culled = base["special"]["culled"]
    assert np.abs(ref["dL_dsh"]).max() > 0 and np.abs(ref["dL_dsh"][-1]).max() > 0
    for v in ("base",) + L.variants("deg3"):
        sc = L.get("deg3", v)
        got = _layout_call(sc, gpu, mode)
        assert got["dL_dsh"].shape == (L.P, sc["M"], 3)
        sh_ref = dict(ref, dL_dsh=ref["dL_dsh"][:, :min(sc["M"], 16)])
        got16 = dict(got, dL_dsh=got["dL_dsh"][:, :min(sc["M"], 16)])
        _same_bits(got16, sh_ref, f"{sc['name']}/{mode}")
        assert (got["dL_dsh"][:, 16:] == 0).all(), sc["name"]  # (M = 25: columns 16 .. 24)
        for k, t in got.items():
            assert np.isfinite(t).all(), (sc["name"], k)
            if k not in CAMERA_NAMES:
                assert (t[culled] == 0).all(), (sc["name"], k)
    # entries above the active degree: degree 2 of the same geometry, 16-coefficient rows
    low = L.get("deg2")
    got = _layout_call(low, gpu, mode)
    assert (got["dL_dsh"][:, 9:] == 0).all() and np.abs(got["dL_dsh"][:, :9]).max() > 0
    _same_bits(_layout_call(L.get("deg2", "poison"), gpu, mode), got, f"deg2/poison/{mode}")


# ---- 4 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("plain", "all"))
def test_equals_the_atomic_path_in_eight_parts(mode, gpu):
    """S1's geometry (sh_layout_scenes deg3), the gradient on one part of dL_masks at a time: a
    row has at most two non-zero addends, so both paths are exact up to one rounding."""
    sc = L.get("deg3")
    reached = 0
    for part in range(len(L.dL_masks())):
        det = _layout_call(sc, gpu, mode, part=part)
        _same_bits(det, _layout_call(sc, gpu, mode, det=False, part=part), f"{mode}, part {part}")
        reached += np.abs(det["dL_dmeans3D"]).max(axis=1) > 0
    assert (reached > 0).sum() >= 40 and (reached > 1).sum() >= 10


@pytest.mark.parametrize("name,tile_x,tile_y,quad", fs.PLACEMENTS)
def test_equals_the_atomic_path_in_one_quadrant(name, tile_x, tile_y, quad, gpu):
    """The gradient confined to one 8 x 8 quadrant: one addend per row.  The default call's bits
    in every tensor, and zeros for every Gaussian outside that tile's list: a store to a wrong
    slot, or a slot gathered into a wrong row, cannot pass."""
    sc = fs.get(name)
    fwd = _fwd(sc, gpu)
    dL = fs.localized(sc, tile_x, tile_y, quad)
    det = _call(sc, gpu, dL)
    _same_bits(det, _call(sc, gpu, dL, det=False), f"{name} ({tile_x}, {tile_y}) quadrant {quad}")
    tile = tile_y * ((sc["W"] + 15) // 16) + tile_x
    r0, r1 = (int(v) for v in fwd["ranges"][tile])
    listed = np.zeros(len(sc["s"]["g"].xyz), bool)
    listed[fwd["point_list"][r0:r1].astype(np.int64)] = True
    assert 0 < listed.sum() < len(listed)
    for k, v in det.items():
        assert _is_zero(v[~listed]), k
    assert np.abs(det["dL_dmeans3D"][listed]).max() > 0


# ---- 5 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("colour", "all_aa"))
@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_accuracy_toy_scenes(name, kind, gpu):
    """S1-S4 within 8 x f of the float64 reference: grad_reference's bounds for the colour loss,
    aa_reference's for colour + planes + camera, antialiased (test_gpu_backward's and
    test_gpu_antialiasing's own checks, on the deterministic call)."""
    sc = grad_scenes.get(name)
    if kind == "colour":
        got = _f64(_call(sc, gpu, sc["dL"], conic=False))
        _assert_end_to_end(got, _toy_reference(sc, gpu), f"{name}/deterministic")
    else:
        sc = aa_scenes.get(name)
        ref = _aa_reference(sc, gpu, "combined")
        dL, dLp = ar.loss_gradients(sc, "combined")
        got = _f64(_call(sc, gpu, dL, dLp, camera=True, aa=True, conic=False))
        _aa_assert_close(got, ref, f"{name}/combined/deterministic")
    assert (got["dL_dmeans2D"][:, 2] == 0).all()


@pytest.mark.parametrize("name,kind", [(n, "colour") for n in fs.NAMES] + [("frame", "all_aa")])
def test_accuracy_frames(name, kind, gpu):
    """frame, wall, wide, tall under the masked gradients within frame_grad_scenes.bound."""
    sc = fs.get(name)
    _fwd(sc, gpu)
    ref = fs.reference(sc, kind)
    if kind == "colour":
        got = _f64(_call(sc, gpu, fs.masked(sc, planes=False)[0], conic=False))
        _all_close(got, ref, name, kind, f"{name}/{kind}/deterministic")
    else:
        dL, dLp = fs.masked(sc)
        got = _f64(_call(sc, gpu, dL, dLp, camera=True, aa=True, conic=False))
        _all_close(got, ref, name, kind, f"{name}/{kind}/deterministic", END_TO_END + CAMERA)
    culled = fs.oracle_of(sc)["radii"] == 0
    for k, v in got.items():
        if k not in CAMERA_NAMES:
            assert (v[culled] == 0).all(), k


# ---- 6 --------------------------------------------------------------------------------------------
def test_exact_zeros(gpu):
    """wall: the Gaussians no pixel composites own slots nothing is stored to -- zeros from the
    gather (dL_dconic, and dL_dcolors with precomputed colours, the blend's own sums) while the
    composited ones of the near layer are not, and zeros (of either sign: the per-Gaussian stage
    multiplies a zero row by signed factors) in every tensor; culled Gaussians, of S4 and of frame,
    exact zeros in every tensor."""
    sc = fs.get("wall")
    fwd = _fwd(sc, gpu)
    comp = fs.composited(sc)
    assert (~comp).sum() >= 100
    dL, dLp = fs.masked(sc)
    got = _call(sc, gpu, dL, colors=fwd["rgb"])
    front = sc["special"]["front"][comp[sc["special"]["front"]]]
    for k in ("dL_dconic", "dL_dcolors"):
        assert _is_zero(got[k][~comp]), k
        assert (np.abs(got[k][front]).max(axis=1) > 0).all(), k
    got = _call(sc, gpu, dL, dLp, aa=True)
    for k, v in got.items():
        assert _is_zero(v[~comp]), k
    edges, frame = grad_scenes.get("edges"), fs.get("frame")
    for s2, least in ((edges, 4), (frame, 1)):
        culled = np.asarray(fs.oracle_of(s2)["radii"]) == 0
        assert culled.sum() >= least
        dLp2 = np.ascontiguousarray(np.random.default_rng(5).standard_normal(
            (3, s2["H"], s2["W"])), np.float32)
        for k, v in _call(s2, gpu, s2["dL"], dLp2, camera=True, aa=True).items():
            if k not in CAMERA_NAMES:
                assert (v[culled] == 0).all(), (s2["name"], k)


# ---- 7 --------------------------------------------------------------------------------------------
def test_buffer_reuse_on_one_context(gpu):
    """One fresh context through frame (K of 117-tile rects), S1, frame with the camera, wide, S1:
    the slots, the marks and the slab shrink and grow; every result has the bits of the same call
    on a context of its own."""
    frame, wide, chain = fs.get("frame"), fs.get("wide"), grad_scenes.get("chain")
    calls = (("1 frame", lambda s: _call(frame, gpu, frame["dL"], slot=s)),
             ("2 chain", lambda s: _call(chain, gpu, chain["dL"], slot=s)),
             ("3 frame, camera", lambda s: _call(frame, gpu, frame["dL"], frame["dLp"],
                                                 camera=True, slot=s)),
             ("4 wide", lambda s: _call(wide, gpu, wide["dL"], slot=s)),
             ("5 chain", lambda s: _call(chain, gpu, chain["dL"], slot=s)))
    slot = _new_slot()
    for what, call in calls:
        _same_bits(call(slot), call(_new_slot()), what)


# ---- 8 --------------------------------------------------------------------------------------------
def _autograd_twice(sc, gpu, **settings):
    """Two forward + backward passes through GaussianRasterizer under the dense colour loss; the
    .grad of every leaf after each."""
    s = sc["s"]
    runs = []
    for _ in range(2):
        d = _inputs(sc, gpu)
        for v in d.values():
            if v is not None:
                v.requires_grad_(True)
        means2D = torch.zeros_like(d["means3D"], requires_grad=True)
        view = to_dev(s["view"], gpu).requires_grad_(True)
        rs = GaussianRasterizationSettings(
            sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"], view,
            to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu), False, False,
            **settings)
        color, _ = GaussianRasterizer(rs)(means2D=means2D, **d)
        (color * to_dev(sc["dL"], gpu)).sum().backward()
        runs.append({k: t.grad.cpu().numpy() for k, t in
                     dict(d, means2D=means2D, view=view).items() if t is not None})
    return runs


def test_every_entry(gpu):
    sc = fs.get("frame")
    s, d = sc["s"], _inputs(sc, gpu)
    # ctypes: _call; the extension's general entry with its 23rd argument
    e = torch.empty(0)
    ext = lambda *more: _C.rasterize_gaussians_backward_ext(  # noqa: E731
        to_dev(s["bg"], gpu), d["means3D"], e, d["opacities"], d["scales"], d["rotations"],
        s["scale_modifier"], e, to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["tx"], s["ty"],
        d["shs"], s["sh_degree"], to_dev(s["campos"], gpu), False, to_dev(sc["dL"], gpu), e, e, e,
        True, False, *more)
    a, b = ext(True), ext(True)
    assert len(a) == 11
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    by_ctypes = _call(sc, gpu, sc["dL"], camera=True, conic=False)
    names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
             "dL_dscales", "dL_drotations", "dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos")
    for n, x in zip(names, a):
        np.testing.assert_array_equal(_bits(x.cpu().numpy().reshape(by_ctypes[n].shape)),
                                      _bits(by_ctypes[n]), err_msg=n)
    # (the 22-argument call still stands, and is the default path: within rounding of the other)
    c = ext()
    assert len(c) == 11
    assert float((c[3] - a[3]).abs().max()) <= 1e-4 * float(a[3].abs().max())
    # GaussianRasterizer: the setting, then None under torch's switch
    first, second = _autograd_twice(sc, gpu, deterministic=True)
    _same_bits(second, first, "GaussianRasterizer(deterministic=True)")
    np.testing.assert_array_equal(_bits(first["means3D"]), _bits(by_ctypes["dL_dmeans3D"]))
    np.testing.assert_array_equal(_bits(first["view"]), _bits(by_ctypes["dL_dviewmatrix"]))
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        third, fourth = _autograd_twice(sc, gpu)
    finally:
        torch.use_deterministic_algorithms(was)
    _same_bits(fourth, third, "torch.use_deterministic_algorithms(True)")
    _same_bits(third, first, "the setting and the switch")


# ---- 9, 10 ------------------------------------------------------------------------------------------
SENTINEL = -559038737  # 0xDEADBEEF as int32


def _raw(sc, gpu, order, dL, strip=False, P=None, camera=True, slot=0):
    """gsr_backward_ordered through the C ABI with sentinel-filled outputs: (rc, the gradients
    and the camera's three as int32 views)."""
    lib = _lib.load_library()
    s, d = sc["s"], _inputs(sc, gpu)
    n = len(s["g"].xyz) if P is None else P
    g = _lib.GsrGaussians(P=n, D=s["sh_degree"], M=16, scale_modifier=s["scale_modifier"],
                          means3D=d["means3D"].data_ptr(), scales=d["scales"].data_ptr(),
                          rotations=d["rotations"].data_ptr(), opacities=d["opacities"].data_ptr(),
                          shs=d["shs"].data_ptr())
    held = [to_dev(s[k], gpu) for k in ("view", "proj", "campos", "bg")]
    st = _lib.GsrRasterSettings(image_width=sc["W"], image_height=sc["H"], tanfovx=s["tx"],
                                tanfovy=s["ty"], viewmatrix=held[0].data_ptr(),
                                projmatrix=held[1].data_ptr(), campos=held[2].data_ptr(),
                                bg=held[3].data_ptr(), tile_row_begin=0,
                                tile_row_end=1 if strip else 0)
    full = len(s["g"].xyz)
    out = {k: torch.full((full, w), SENTINEL, dtype=torch.int32, device=gpu) for k, w in
           (("dL_dmeans3D", 3), ("dL_dmeans2D", 3), ("dL_dopacity", 1), ("dL_dsh", 48),
            ("dL_dscales", 3), ("dL_drotations", 4))}
    cam = {k: torch.full((w,), SENTINEL, dtype=torch.int32, device=gpu)
           for k, w in (("dL_dviewmatrix", 16), ("dL_dprojmatrix", 16), ("dL_dcampos", 3))}
    dLd = to_dev(dL, gpu)
    rc = _lib.backward_ordered_fn(lib)(
        _lib.context(gpu.index or 0, slot), ctypes.byref(g), ctypes.byref(st),
        ctypes.byref(_lib.GsrBackwardInputs(dL_dcolor=dLd.data_ptr())), None,
        ctypes.byref(_lib.GsrCameraGradients(**{k: t.data_ptr() for k, t in cam.items()}))
        if camera else None, None,
        None if order is None else ctypes.byref(_lib.GsrBackwardOrder(deterministic=order)),
        ctypes.byref(_lib.GsrGradients(**{k: t.data_ptr() for k, t in out.items()})),
        ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    torch.cuda.synchronize(gpu)
    return rc, {k: t.cpu().numpy() for k, t in {**out, **cam}.items()}


def test_errors(gpu):
    sc = grad_scenes.get("chain")
    lib = _lib.load_library()
    for order in (2, -1):
        rc, out = _raw(sc, gpu, order, sc["dL"])
        assert rc == -1 and b"deterministic must be 0 or 1" in lib.gsr_last_error()
        assert all((v == SENTINEL).all() for v in out.values())
    for order in (1, 0, None):
        rc, out = _raw(sc, gpu, order, sc["dL"], strip=True)
        assert rc == -1 and b"whole frames only" in lib.gsr_last_error()
        assert all((v == SENTINEL).all() for v in out.values())
    rc, out = _raw(sc, gpu, 1, sc["dL"], P=0)
    assert rc == 0
    for k in CAMERA_NAMES:
        assert (out[k] == 0).all(), k
    assert (out["dL_dmeans3D"] == SENTINEL).all()
    # ... and the plain call fills what the failed ones left
    rc, out = _raw(sc, gpu, 1, sc["dL"])
    assert rc == 0 and not any((v == SENTINEL).any() for v in out.values())
    ref = _call(sc, gpu, sc["dL"], camera=True)
    for k, v in out.items():
        np.testing.assert_array_equal(v.view(np.uint32).reshape(-1), _bits(ref[k]).reshape(-1), k)


@pytest.mark.parametrize("order", (None, 0))
def test_off_means_untouched(order, gpu):
    """A NULL order and deterministic = 0 are gsr_backward_filtered, checked as
    test_gpu_function_paths.py checks its routes, by what the route computes: on a gradient
    confined to one quadrant (one addend per row, so the default path is reproducible) that
    entry's bits in every tensor, the camera's included; under the masked dense gradient the
    float64 reference's bound, like every default call."""
    sc = fs.get("frame")
    _fwd(sc, gpu)
    slot = _new_slot()
    dL = fs.localized(sc, 6, 4, 3)
    rc, out = _raw(sc, gpu, order, dL, slot=slot)
    assert rc == 0
    ref = _call(sc, gpu, dL, camera=True, det=False, conic=False, slot=slot)
    for k, v in out.items():
        np.testing.assert_array_equal(v.view(np.uint32).reshape(-1), _bits(ref[k]).reshape(-1), k)
    rc, out = _raw(sc, gpu, order, fs.masked(sc, planes=False)[0], slot=slot)
    assert rc == 0
    got = {k: v.view(np.float32).astype(np.float64).reshape(ref[k].shape) for k, v in out.items()}
    _all_close(got, fs.reference(sc, "colour"), "frame", "colour", f"order = {order}")
