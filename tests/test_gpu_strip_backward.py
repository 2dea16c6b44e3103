"""GPU: the backward on tile row strips (gsr_backward_strip) on the strips of
strip_grad_scenes: the whole frame's backward with the image gradients zero outside the strip's
pixel rows, with strip-local inputs and whole-scene outputs.

Per gradient tensor e = max|g_gpu - g_ref64| / max|g_ref64| (the camera's three: cam_err) against
the strip's own float64 reference must stay within 8 x f, f the strip reference's float32 spread
(strip_grad_scenes.F32_SPREAD, measured on the CPU).

  1 every strip, default mode, the colour loss: every gradient within its bound
  2 frame's strips with planes + camera, and antialiased: the same, the camera's three included
  3 zeros: every Gaussian without a tile in the strip has +-0.0 bits in every gradient, both modes
  4 deterministic mode, every strip: equal bits on two fresh contexts with an unrelated frame in
    between; Gaussians wholly inside the strip have the bits of the whole-frame
    gsr_backward_ordered call under the strip-masked full-size image gradient; the strip
    (0, grid_y) has those bits for everything, the camera included; the whole result (the clipped
    Gaussians among it) within check 1's bound
  5 the strips' deterministic gradients added on the host in float64 against the whole frame's,
    within the sum of the strips' absolute allowances plus the whole frame's (the triangle
    inequality through the references, which add up exactly: test_strip_grad_reference.py)
  6 the strip forward's bits: GaussianRasterizer(tile_rows=) gives rasterize_gaussians_native(
    tile_rows=)'s colour and planes; autograd through it equals the ctypes call in deterministic
    mode bit for bit (tall (1, 257) among them)
  7 bands: frame's three strips in a loop, each loss.backward() accumulating into .grad,
    deterministic: two runs, equal bits
  8 errors: a bad strip is GSR_E_INVALID with nothing written; a wrong image gradient shape raises;
    an old entry still refuses a strip; gsr_get_binning after a strip backward exports the strip
    forward's upstream lists
"""
import ctypes

import numpy as np
import pytest
import torch

import frame_grad_scenes as fs
import plane_grad_reference as pg
import strip_grad_scenes as ss
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import (PLANE_NAMES, GaussianRasterizationSettings,
                                                    GaussianRasterizer, binning_state,
                                                    rasterize_gaussians_backward_native,
                                                    rasterize_gaussians_native)
from gpu_helpers import run_hip, to_dev
from test_gpu_backward import END_TO_END, _inputs
from test_gpu_backward_frames import CAMERA, _fwd, _is_zero

pytestmark = pytest.mark.gpu

CAMERA_NAMES = tuple(n for n, _ in CAMERA)
# (context slots of this file alone; test_gpu_deterministic_backward.py hands out 500 upwards)
_next_slot = [600]
_runs = {}  # (scene, strip, kind, deterministic) -> the call's gradients on slot 0


def _new_slot():
    _next_slot[0] += 1
    return _next_slot[0]


def _call(sc, gpu, strip, kind, det, slot=0, dL=None, dLp=None):
    """One native backward as float32 numpy arrays by their gsr_gradients names.  strip None: the
    whole frame (gsr_backward_ordered / _filtered) under the given full-size dL, dLp; else
    gsr_backward_strip under the strip-local masked gradients."""
    s, d = sc["s"], _inputs(sc, gpu)
    planes = kind != "colour"
    kw = {}
    if strip is not None:
        dL, dLp = ss.local_dL(sc, strip, planes)
        kw = dict(tile_rows=strip, image_height=sc["H"])
    if planes:
        kw.update({f"dL_d{n}": to_dev(dLp[i], gpu) for i, n in enumerate(pg.PLANES)})
        kw["depths"] = True
    g = rasterize_gaussians_backward_native(
        to_dev(s["bg"], gpu), d["means3D"], d["colors_precomp"], d["opacities"], d["scales"],
        d["rotations"], s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], to_dev(dL, gpu), d["shs"], s["sh_degree"],
        to_dev(s["campos"], gpu), camera=planes, antialiasing=kind == "all_aa", slot=slot,
        deterministic=det, **kw)
    return {k: v.cpu().numpy() for k, v in g.items()}


def _run(name, strip, kind, det, gpu):
    key = (name, strip, kind, det)
    if key not in _runs:
        sc = fs.get(name)
        _fwd(sc, gpu)  # the GPU forward's lists, radii and records are the oracle's
        _runs[key] = _call(sc, gpu, strip, kind, det)
    return _runs[key]


def _f64(got):
    out = {k: v.astype(np.float64) for k, v in got.items()}
    if "dL_dcampos" in out:
        out["dL_dcampos"] = out["dL_dcampos"].reshape(-1)[:3]
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, ref, what, rows=None):
    assert set(got) == set(ref), what
    for k, v in got.items():
        w = ref[k]
        if rows is not None:
            if k in CAMERA_NAMES:
                continue
            v, w = v[rows], w[rows]
        bad = _bits(v) != _bits(w)
        assert not bad.any(), f"{what}: {k} differs in {bad.sum()} words"


def _pairs(kind):
    return END_TO_END if kind == "colour" else END_TO_END + CAMERA


def _assert_close(got, name, strip, kind, what):
    ref = ss.reference(fs.get(name), strip, kind)
    got = _f64(got)
    bad, seen = [], 0
    for out, key in _pairs(kind):
        if key in ref and out in got and key in ss.F32_SPREAD[(name, strip, kind)]:
            e, b = fs.err(got[out], ref, key), ss.bound(name, strip, kind, key)
            print(f"{what}: e[{key}] = {e:.3e} = {e / b:.3f} of the bound {b:.1e}")
            if not e <= b:
                bad.append(f"{what}: e[{key}] = {e:.3e} > {b:.1e}")
            seen += 1
    assert seen >= (6 if kind == "colour" else 9) and not bad, bad
    assert (got["dL_dmeans2D"][:, 2] == 0).all()


ALL_RUNS = [(n, s, k) for n, s in ss.CASES for k in ss.KINDS[n]]


# ---- 1, 2 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,strip", ss.CASES)
def test_default_mode_colour(name, strip, gpu):
    _assert_close(_run(name, strip, "colour", False, gpu), name, strip, "colour",
                  f"{name} {strip}/colour")


@pytest.mark.parametrize("kind", ("all", "all_aa"))
@pytest.mark.parametrize("strip", ss.STRIPS["frame"])
def test_default_mode_planes_camera(strip, kind, gpu):
    got = _run("frame", strip, kind, False, gpu)
    assert set(CAMERA_NAMES) <= set(got) and "dL_ddepths" in got
    _assert_close(got, "frame", strip, kind, f"frame {strip}/{kind}")


# ---- 3 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", (False, True), ids=("default", "deterministic"))
@pytest.mark.parametrize("name,strip,kind", ALL_RUNS)
def test_zeros_without_a_tile_in_the_strip(name, strip, kind, det, gpu):
    sc = fs.get(name)
    got = _run(name, strip, kind, det, gpu)
    inside, clipped, none = ss.classes(sc, strip)
    assert none.sum() >= 1 or name == "wall"
    for k, v in got.items():
        assert np.isfinite(v).all(), k
        if k not in CAMERA_NAMES:
            assert _is_zero(v[none]), k
    # ... and the others are reached
    assert np.abs(got["dL_dmeans3D"][inside | clipped]).max() > 0
    culled = np.asarray(fs.oracle_of(sc)["radii"]) == 0
    assert (none | ~culled).all()


# ---- 4 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,strip,kind", ALL_RUNS)
def test_deterministic_accuracy(name, strip, kind, gpu):
    """The whole result, the clipped Gaussians among it, within the default mode's bound."""
    _assert_close(_run(name, strip, kind, True, gpu), name, strip, kind,
                  f"{name} {strip}/{kind}/deterministic")


@pytest.mark.parametrize("name,strip", ss.CASES)
def test_deterministic_bits(name, strip, gpu):
    sc = fs.get(name)
    kind = ss.KINDS[name][-1]
    first = _call(sc, gpu, strip, kind, True, _new_slot())
    # an unrelated frame, forward and backward in both modes, on the second context in between
    other = fs.get("wall" if name != "wall" else "frame")
    slot = _new_slot()
    run_hip(other["s"], gpu, slot=slot)
    _call(other, gpu, None, "colour", False, slot, dL=other["dL"])
    _call(other, gpu, ss.STRIPS[other["name"]][0], "colour", True, slot)
    _same_bits(_call(sc, gpu, strip, kind, True, slot), first, f"{name} {strip}: two contexts")
    _same_bits(_run(name, strip, kind, True, gpu), first, f"{name} {strip}: slot 0")
    # wholly inside the strip: the whole frame's deterministic bits under the masked gradient
    dL, dLp = ss.full_dL(sc, strip, kind != "colour")
    whole = _call(sc, gpu, None, kind, True, dL=dL, dLp=dLp)
    inside, clipped, _ = ss.classes(sc, strip)
    assert inside.sum() >= 1 or name == "wall"
    _same_bits(first, whole, f"{name} {strip}: wholly inside", rows=inside)
    assert inside.sum() == 0 or np.abs(whole["dL_dmeans3D"][inside]).max() > 0


@pytest.mark.parametrize("name", list(ss.STRIPS))
def test_the_full_strip_is_the_whole_frame(name, gpu):
    """(0, grid_y): the whole-frame deterministic bits for every Gaussian and for the camera."""
    sc = fs.get(name)
    kind = ss.KINDS[name][-1]
    strip = (0, ss.grid(sc)[1])
    dL, dLp = fs.masked(sc, kind != "colour")
    _same_bits(_call(sc, gpu, strip, kind, True), _call(sc, gpu, None, kind, True, dL=dL, dLp=dLp),
               f"{name} {strip}")


# ---- 5 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [(n, k) for n in ss.STRIPS for k in ss.KINDS[n]])
def test_strips_add_up(name, kind, gpu):
    sc = fs.get(name)
    dL, dLp = fs.masked(sc, kind != "colour")
    whole = _f64(_call(sc, gpu, None, kind, True, dL=dL, dLp=dLp))
    parts = [_f64(_run(name, strip, kind, True, gpu)) for strip in ss.STRIPS[name]]
    ref_whole = fs.reference(sc, kind)
    bad, seen = [], 0

    def scale(ref, key):  # what fs.err divides by
        return ref["S"][key] if key in ("viewmatrix", "projmatrix", "campos") else \
            float(np.abs(ref[key]).max())

    for out, key in _pairs(kind):
        if key not in ref_whole or out not in whole or key not in fs.F32_SPREAD[(name, kind)]:
            continue
        allow = fs.bound(name, kind, key) * scale(ref_whole, key)
        for strip in ss.STRIPS[name]:
            allow += ss.bound(name, strip, kind, key) * scale(ss.reference(sc, strip, kind), key)
        total = sum(p[out] for p in parts)
        d = float(np.abs(total.reshape(-1) - whole[out].reshape(-1)).max())
        print(f"{name}/{kind}: |sum - whole|[{key}] = {d:.3e} = {d / allow:.3f} of {allow:.3e}")
        if not d <= allow:
            bad.append((key, d, allow))
        seen += 1
    assert seen >= (6 if kind == "colour" else 9) and not bad, bad


# ---- 6, 7 -----------------------------------------------------------------------------------------
def _rasterizer_run(sc, gpu, strip, dL_local, depth_maps=False, accumulate=None, **settings):
    """Forward + backward through GaussianRasterizer(tile_rows=strip) under (color * dL).sum();
    returns (outputs, the leaves).  accumulate: leaves of an earlier run to add .grad into."""
    s = sc["s"]
    if accumulate is None:
        d = _inputs(sc, gpu)
        for v in d.values():
            if v is not None:
                v.requires_grad_(True)
        leaves = dict(d, means2D=torch.zeros_like(d["means3D"], requires_grad=True),
                      view=to_dev(s["view"], gpu).requires_grad_(True))
    else:
        leaves = accumulate
    d = {k: v for k, v in leaves.items() if k not in ("means2D", "view")}
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
        leaves["view"], to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu), False,
        False, depth_maps=depth_maps, tile_rows=strip, **settings)
    out = GaussianRasterizer(rs)(means2D=leaves["means2D"], **d)
    (out[0] * to_dev(dL_local, gpu)).sum().backward()
    return out, leaves


def _grads(leaves):
    return {k: t.grad.cpu().numpy() for k, t in leaves.items() if t is not None}


@pytest.mark.parametrize("name,strip", [("frame", (3, 8)), ("frame", (8, 9)), ("tall", (1, 257))])
def test_rasterizer_strip_forward_and_autograd(name, strip, gpu):
    sc = fs.get(name)
    s, d = sc["s"], _inputs(sc, gpu)
    y0, y1 = ss.pixel_rows(sc, strip)
    dL = np.ascontiguousarray(sc["dL"][:, y0:y1])
    out, leaves = _rasterizer_run(sc, gpu, strip, dL, depth_maps=True, deterministic=True)
    assert len(out) == 5 and out[0].shape == (3, y1 - y0, sc["W"])
    assert out[1].shape == (len(s["g"].xyz),)
    nat = rasterize_gaussians_native(
        to_dev(s["bg"], gpu), d["means3D"], None, d["opacities"], d["scales"], d["rotations"],
        s["scale_modifier"], None, to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["tx"],
        s["ty"], sc["H"], sc["W"], d["shs"], s["sh_degree"], to_dev(s["campos"], gpu), False,
        False, tile_rows=strip, extras=PLANE_NAMES)
    assert torch.equal(out[0].detach().view(torch.int32), nat.color.view(torch.int32))
    assert torch.equal(out[1], nat.radii)
    for i, n in enumerate(PLANE_NAMES):
        assert out[2 + i].shape == (y1 - y0, sc["W"])
        assert torch.equal(out[2 + i].detach().view(torch.int32), nat.extras[n].view(torch.int32)), n
    # autograd (the camera's Function: view requires a gradient) against the ctypes call
    g = rasterize_gaussians_backward_native(
        to_dev(s["bg"], gpu), d["means3D"], None, d["opacities"], d["scales"], d["rotations"],
        s["scale_modifier"], None, to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["tx"],
        s["ty"], to_dev(dL, gpu), d["shs"], s["sh_degree"], to_dev(s["campos"], gpu), camera=True,
        deterministic=True, tile_rows=strip, image_height=sc["H"])
    got = _grads(leaves)
    for leaf, k in (("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"),
                    ("opacities", "dL_dopacity"), ("shs", "dL_dsh"), ("scales", "dL_dscales"),
                    ("rotations", "dL_drotations"), ("view", "dL_dviewmatrix")):
        np.testing.assert_array_equal(_bits(got[leaf]).reshape(-1),
                                      _bits(g[k].cpu().numpy()).reshape(-1), err_msg=k)
    assert np.abs(got["means3D"]).max() > 0 and np.abs(got["view"]).max() > 0
    # ... and the plain Function (no camera leaf), default mode: within rounding of it
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu),
        False, False, tile_rows=strip)
    x = d["means3D"].clone().requires_grad_(True)
    color, _ = GaussianRasterizer(rs)(means3D=x, means2D=None, **{k: v for k, v in d.items()
                                                                 if k != "means3D"})
    assert torch.equal(color.detach().view(torch.int32), nat.color.view(torch.int32))
    (color * to_dev(dL, gpu)).sum().backward()
    m = float(np.abs(got["means3D"]).max())
    assert float(np.abs(x.grad.cpu().numpy() - got["means3D"]).max()) <= 1e-4 * m


def test_bands_accumulate_reproducibly(gpu):
    sc = fs.get("frame")
    runs = []
    for _ in range(2):
        leaves = None
        for strip in ss.STRIPS["frame"]:
            y0, y1 = ss.pixel_rows(sc, strip)
            _, leaves = _rasterizer_run(sc, gpu, strip, np.ascontiguousarray(sc["dL"][:, y0:y1]),
                                        accumulate=leaves, deterministic=True)
        runs.append(_grads(leaves))
    _same_bits(runs[1], runs[0], "frame: three bands accumulated")
    # the accumulated gradient is the whole frame's up to rounding
    dense = _call(sc, gpu, None, "colour", True, dL=sc["dL"])
    m = float(np.abs(dense["dL_dmeans3D"]).max())
    assert float(np.abs(runs[0]["means3D"] - dense["dL_dmeans3D"]).max()) <= 1e-4 * m


def test_shading_still_has_no_backward(gpu):
    sc = fs.get("wall")
    s, d = sc["s"], _inputs(sc, gpu)
    x = d["means3D"].clone().requires_grad_(True)
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu),
        False, False, _lib.GSR_SHADE_FLAT_BALL, tile_rows=(1, 2))
    color, _ = GaussianRasterizer(rs)(means3D=x, means2D=None, **{k: v for k, v in d.items()
                                                                 if k != "means3D"})
    assert color.shape == (3, 16, 32)
    with pytest.raises(RuntimeError, match="splat composite\\s+only"):
        color.sum().backward()


# ---- 8 --------------------------------------------------------------------------------------------
SENTINEL = -559038737  # 0xDEADBEEF as int32


def _raw(sc, gpu, fn, strip, dL, order=1, slot=0):
    """A backward entry through the C ABI with sentinel-filled outputs: (rc, the gradients and the
    camera's three as int32 views)."""
    s, d = sc["s"], _inputs(sc, gpu)
    P = len(s["g"].xyz)
    g = _lib.GsrGaussians(P=P, D=s["sh_degree"], M=16, scale_modifier=s["scale_modifier"],
                          means3D=d["means3D"].data_ptr(), scales=d["scales"].data_ptr(),
                          rotations=d["rotations"].data_ptr(), opacities=d["opacities"].data_ptr(),
                          shs=d["shs"].data_ptr())
    held = [to_dev(s[k], gpu) for k in ("view", "proj", "campos", "bg")]
    st = _lib.GsrRasterSettings(image_width=sc["W"], image_height=sc["H"], tanfovx=s["tx"],
                                tanfovy=s["ty"], viewmatrix=held[0].data_ptr(),
                                projmatrix=held[1].data_ptr(), campos=held[2].data_ptr(),
                                bg=held[3].data_ptr(), tile_row_begin=strip[0],
                                tile_row_end=strip[1])
    out = {k: torch.full((P, w), SENTINEL, dtype=torch.int32, device=gpu) for k, w in
           (("dL_dmeans3D", 3), ("dL_dmeans2D", 3), ("dL_dopacity", 1), ("dL_dsh", 48),
            ("dL_dscales", 3), ("dL_drotations", 4))}
    cam = {k: torch.full((w,), SENTINEL, dtype=torch.int32, device=gpu)
           for k, w in (("dL_dviewmatrix", 16), ("dL_dprojmatrix", 16), ("dL_dcampos", 3))}
    dLd = to_dev(dL, gpu)
    rc = fn(_lib.context(gpu.index or 0, slot), ctypes.byref(g), ctypes.byref(st),
            ctypes.byref(_lib.GsrBackwardInputs(dL_dcolor=dLd.data_ptr())), None,
            ctypes.byref(_lib.GsrCameraGradients(**{k: t.data_ptr() for k, t in cam.items()})),
            None, ctypes.byref(_lib.GsrBackwardOrder(deterministic=order)),
            ctypes.byref(_lib.GsrGradients(**{k: t.data_ptr() for k, t in out.items()})),
            ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    torch.cuda.synchronize(gpu)
    return rc, {k: t.cpu().numpy() for k, t in {**out, **cam}.items()}


def test_errors(gpu):
    sc = fs.get("frame")
    lib = _lib.load_library()
    strip_fn = _lib.backward_strip_fn(lib)
    dL = ss.local_dL(sc, (3, 8), False)[0]
    for bad in ((-1, 3), (0, 10), (4, 4), (5, 2)):
        for order in (0, 1):
            rc, out = _raw(sc, gpu, strip_fn, bad, dL, order)
            assert rc == -1 and b"bad tile row strip" in lib.gsr_last_error(), bad
            assert all((v == SENTINEL).all() for v in out.values()), bad
    # an old entry still refuses a strip
    rc, out = _raw(sc, gpu, _lib.backward_ordered_fn(lib), (3, 8), dL)
    assert rc == -1 and b"whole frames only" in lib.gsr_last_error()
    assert all((v == SENTINEL).all() for v in out.values())
    # ... and the good call fills what the failed ones left, with the Python entry's bits
    rc, out = _raw(sc, gpu, strip_fn, (3, 8), dL)
    assert rc == 0 and not any((v == SENTINEL).any() for v in out.values())
    s, d = sc["s"], _inputs(sc, gpu)
    args = (to_dev(s["bg"], gpu), d["means3D"], None, d["opacities"], d["scales"], d["rotations"],
            s["scale_modifier"], None, to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["tx"],
            s["ty"])
    tail = (d["shs"], s["sh_degree"], to_dev(s["campos"], gpu))
    ref = rasterize_gaussians_backward_native(*args, to_dev(dL, gpu), *tail, camera=True,
                                              deterministic=True, tile_rows=(3, 8),
                                              image_height=sc["H"])
    for k, v in out.items():
        np.testing.assert_array_equal(v.view(np.uint32).reshape(-1),
                                      _bits(ref[k].cpu().numpy()).reshape(-1), k)
    # a wrong image gradient shape raises: the whole frame's, another strip's
    for wrong in (sc["dL"], ss.local_dL(sc, (8, 9), False)[0]):
        with pytest.raises(RuntimeError, match="must have 80 rows"):
            rasterize_gaussians_backward_native(*args, to_dev(wrong, gpu), *tail, tile_rows=(3, 8),
                                                image_height=sc["H"])
    with pytest.raises(RuntimeError, match="tile_rows needs image_height"):
        rasterize_gaussians_backward_native(*args, to_dev(dL, gpu), *tail, tile_rows=(3, 8))


@pytest.mark.parametrize("name,strip", [("frame", (3, 8)), ("tall", (1, 257)), ("wall", (1, 2))])
def test_binning_after_a_strip_backward(name, strip, gpu):
    """gsr_get_binning after the strip backward: the strip forward's upstream lists (a forward
    that asks for n_contrib bins those)."""
    sc = fs.get(name)
    slot = _new_slot()
    fwd = run_hip(sc["s"], gpu, tile_rows=strip, slot=slot)
    run_hip(fs.get("wall")["s"], gpu, slot=slot)  # (something else in between)
    _call(sc, gpu, strip, "colour", False, slot)
    pl, pt, rg = (t.cpu().numpy().view(np.uint32) for t in binning_state(gpu.index or 0, slot))
    np.testing.assert_array_equal(pl, fwd["point_list"])
    np.testing.assert_array_equal(pt, fwd["point_tiles"])
    np.testing.assert_array_equal(rg, fwd["ranges"])
    assert len(pl) == fwd["num_rendered"] > 0
    # the lists are the whole frame's inside the strip's tiles
    gx = ss.grid(sc)[0]
    orc = fs.oracle_of(sc)["ranges"].reshape(-1, 2).astype(np.int64)
    got = rg.reshape(-1, 2).astype(np.int64)
    sel = slice(strip[0] * gx, strip[1] * gx)
    np.testing.assert_array_equal(got[sel, 1] - got[sel, 0], orc[sel, 1] - orc[sel, 0])
    assert (got[:sel.start] == 0).all() and (got[sel.stop:] == 0).all()
