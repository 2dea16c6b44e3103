"""GPU: the absolute gradient of the 2D means (gsr_backward_abs) against the float64
reference of absgrad_reference -- per-pixel autograd of grad_reference's restatement on the GPU
forward's own lists and radii -- and the exact properties the kernels owe.

Per tensor e = max|got - ref| / max|ref| must stay within 8 x absgrad_reference.F32_SPREAD, and
every word within 8 x ROW_SPREAD of its own value (both spreads measured on the CPU); a word whose
reference is 0 must be exactly 0.0.  Measured on an MI355X, both orders, every entry: at most
0.095 of the tensor bound (precomputed) and 0.11 of the row bound (chain); the strips' sums within
0.011 of their allowance (README, "Densifying on absolute gradients").

   1 S1-S4 in both orders through ctypes, `_C.rasterize_gaussians_backward_abs` and
     GaussianRasterizer(means2D_abs=): partial quadrants (S1), three chunks per list with capped
     and terminating pixels (S2: the group-of-16 flush, the `open` gate), culled Gaussians (S4)
   2 S1 with the three plane gradients beside the colour (12 sums) and alone (dL_dcolor NULL): a
     wrong word mapping between the 9 / 10 / 11 / 12-sum layouts cannot pass
   3 every other gradient of the call keeps its bits: in the deterministic order always (plain,
     planes, camera, antialiasing), in the default order where a row has at most two addends
   4 exact identities in the deterministic order: one lit pixel gives |dL_dmeans2D| bit for bit;
     negating every image-like gradient changes no bit; two calls, a second stream and another
     frame in between change no bit
   5 the cancellation the output exists for (absgrad_reference.cancellation_scene)
   6 strips: the strips' outputs add up to the frame's, Gaussians without a tile in the strip get
     exact zeros, the deterministic strip (0, grid_y) has the frame's bits
   7 guard words around a 4-byte-aligned output; P = 0 writes nothing
   8 Python: .grad accumulates, the argument's checks, the options it composes with
"""
import ctypes

import numpy as np
import pytest
import torch

import absgrad_reference as ab
import frame_grad_scenes as fs
import grad_reference as gr
import grad_scenes
import plane_grad_reference as pg
import sh_layout_scenes as L
import strip_grad_scenes as ss
from gaussiansplattingviewer_amd import _C, _lib
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer,
                                                    rasterize_gaussians_backward_native)
from gpu_helpers import run_hip, to_dev
from test_gpu_backward import _forward, _inputs
from test_gpu_backward_frames import _fwd

pytestmark = pytest.mark.gpu

CAMERA_NAMES = _lib.CAMERA_GRADIENT_NAMES
ORDERS = pytest.mark.parametrize("det", (False, True), ids=("default", "deterministic"))
# (context slots of this file alone; test_gpu_strip_backward.py hands out 600 upwards)
OTHER_SLOT = 700
_refs = {}
worst = {}  # (scene, loss) -> the largest e / bound seen, per tensor and per row


def _call(sc, gpu, dL, dLp=None, det=False, absgrad=True, strip=None, camera=False, aa=False,
          slot=0, stream=None):
    """One native backward as float32 numpy arrays by their names; dLp: the three planes' gradients
    ([3, rows, W]); strip: (b, e), with dL and dLp strip-local."""
    s, d = sc["s"], _inputs(sc, gpu)
    kw = {}
    if dLp is not None:
        kw = {f"dL_d{n}": to_dev(dLp[i], gpu) for i, n in enumerate(pg.PLANES)}
        kw["depths"] = True
    if strip is not None:
        kw.update(tile_rows=strip, image_height=sc["H"])
    g = rasterize_gaussians_backward_native(
        to_dev(s["bg"], gpu), d["means3D"], d["colors_precomp"], d["opacities"], d["scales"],
        d["rotations"], s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], None if dL is None else to_dev(dL, gpu),
        d["shs"], s["sh_degree"], to_dev(s["campos"], gpu), camera=camera, antialiasing=aa,
        slot=slot, deterministic=det, absgrad=absgrad, stream=stream, **kw)
    return {k: v.cpu().numpy() for k, v in g.items()}


def _reference(name, loss, gpu):
    """absgrad_reference on the GPU forward's lists and radii, once per (scene, loss)."""
    if (name, loss) not in _refs:
        sc = grad_scenes.get(name)
        fwd = _forward(sc, gpu)
        dL, dLp = ab.loss_gradients(sc, loss)
        ref = ab.scene_abs_gradients(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"], dL, dLp)
        assert ref["near"] == (0, 0)
        _refs[(name, loss)] = ref
    return _refs[(name, loss)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, ref, what, skip=()):
    for k in ref:
        if k in skip:
            continue
        bad = _bits(got[k]) != _bits(ref[k])
        assert not bad.any(), f"{what}: {k} differs in {bad.sum()} words"


def _assert_close(got, ref, what, key):
    """got: dL_dmeans2D_abs [P,3]; ref: scene_abs_gradients' dict."""
    got = np.asarray(got, np.float64)
    want = ref["means2D_abs"]
    assert got.shape == want.shape and np.isfinite(got).all()
    assert (got[:, 2] == 0).all() and (got >= 0).all()
    e, (e_row, row) = gr.rel_err(got, want), ab.row_err(got, want)
    w = worst.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], e / ab.bound()), max(w[1], e_row / ab.row_bound())
    print(f"{what}: e = {e:.3e} = {e / ab.bound():.3f} of the bound {ab.bound():.1e}; worst row "
          f"{row}: {e_row:.3e} = {e_row / ab.row_bound():.3f} of the bound {ab.row_bound():.1e}")
    assert (got[want == 0] == 0).all(), f"{what}: a word whose reference is 0 is not 0.0"
    assert e <= ab.bound(), f"{what}: e = {e:.3e} > {ab.bound():.1e}"
    assert e_row <= ab.row_bound(), f"{what}: row {row}: {e_row:.3e} > {ab.row_bound():.1e}"


def _ext(sc, gpu, dL, det, strip=(0, 0), dLp=None, camera=False, aa=False):
    """`_C.rasterize_gaussians_backward_abs`: the 12-tuple."""
    s, d = sc["s"], _inputs(sc, gpu)
    e = torch.empty(0)
    opt = lambda t: e if t is None else t  # noqa: E731
    planes = [e, e, e] if dLp is None else [to_dev(p, gpu) for p in dLp]
    return _C.rasterize_gaussians_backward_abs(
        to_dev(s["bg"], gpu), d["means3D"], opt(d["colors_precomp"]), d["opacities"],
        opt(d["scales"]), opt(d["rotations"]), s["scale_modifier"], opt(d["cov3D_precomp"]),
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["tx"], s["ty"], opt(d["shs"]),
        s["sh_degree"], to_dev(s["campos"], gpu), False, opt(None if dL is None else
                                                             to_dev(dL, gpu)),
        *planes, camera, aa, det, strip[0], strip[1], sc["H"])


def _settings(sc, gpu, **kw):
    s = sc["s"]
    view = kw.pop("view", to_dev(s["view"], gpu))
    return GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"], view,
        to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu), False, False, **kw)


def _autograd(sc, gpu, dL, absgrad=True, **settings):
    """One forward + backward through GaussianRasterizer under sum(color * dL): the .grad of every
    leaf, means2D's and means2D_abs's among them."""
    d = _inputs(sc, gpu)
    for v in d.values():
        if v is not None:
            v.requires_grad_(True)
    P = len(sc["s"]["g"].xyz)
    leaves = dict(d, means2D=torch.zeros((P, 3), device=gpu, requires_grad=True))
    kw = {}
    if absgrad:
        leaves["means2D_abs"] = kw["means2D_abs"] = torch.zeros((P, 3), device=gpu,
                                                                requires_grad=True)
    out = GaussianRasterizer(_settings(sc, gpu, **settings))(means2D=leaves["means2D"], **d, **kw)
    (out[0] * to_dev(dL, gpu)).sum().backward()
    return {k: t.grad.cpu().numpy() for k, t in leaves.items() if t is not None}


# ---- 1 --------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("entry", ("ctypes", "ext", "rasterizer"))
@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_against_the_reference(name, entry, det, gpu):
    sc = grad_scenes.get(name)
    ref = _reference(name, "colour", gpu)
    if entry == "ctypes":
        g = _call(sc, gpu, sc["dL"], det=det)
        got, signed = g["dL_dmeans2D_abs"], g["dL_dmeans2D"]
    elif entry == "ext":
        g = _ext(sc, gpu, sc["dL"], det)
        assert len(g) == 12
        got, signed = g[11].cpu().numpy(), g[0].cpu().numpy()
    else:
        g = _autograd(sc, gpu, sc["dL"], deterministic=det)
        got, signed = g["means2D_abs"], g["means2D"]
    _assert_close(got, ref, f"{name}/{entry}/{'det' if det else 'default'}", (name, "colour"))
    assert np.abs(got).max() > 0
    culled = _forward(sc, gpu)["radii"] == 0
    assert _bits(got[culled]).max(initial=0) == 0  # +0.0, not -0.0
    if name == "edges":
        assert culled.sum() >= 5
    if det:  # fl(sum |v|) >= |fl(sum v)| for one tree of float additions, then one rounding each
        assert (got >= np.abs(signed)).all()


# ---- 2 --------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("loss", ("combined", "planes"))
def test_with_the_planes(loss, det, gpu):
    sc = grad_scenes.get("chain")
    dL, dLp = ab.loss_gradients(sc, loss)
    assert (dL is None) == (loss == "planes")
    g = _call(sc, gpu, dL, dLp, det=det)
    _assert_close(g["dL_dmeans2D_abs"], _reference("chain", loss, gpu),
                  f"chain/{loss}/{'det' if det else 'default'}", ("chain", loss))
    # the planes move it: the colour's reference is another tensor
    colour = _reference("chain", "colour", gpu)["means2D_abs"]
    assert gr.rel_err(g["dL_dmeans2D_abs"], colour) > 100 * ab.bound()
    by_ext = _ext(sc, gpu, dL, det, dLp=dLp)
    if det:
        np.testing.assert_array_equal(_bits(by_ext[11].cpu().numpy()),
                                      _bits(g["dL_dmeans2D_abs"]))


# ---- 3 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("plain", "planes", "camera", "antialiasing"))
def test_deterministic_order_keeps_every_other_bit(kind, gpu):
    sc = grad_scenes.get("chain")
    dLp = pg.plane_dL("chain") if kind in ("planes", "camera") else None
    kw = dict(dLp=dLp, det=True, camera=kind == "camera", aa=kind == "antialiasing")
    with_abs = _call(sc, gpu, sc["dL"], **kw)
    without = _call(sc, gpu, sc["dL"], absgrad=False, **kw)
    assert set(with_abs) == set(without) | {"dL_dmeans2D_abs"}
    assert "dL_dmeans2D_abs" not in without and np.abs(with_abs["dL_dmeans2D_abs"]).max() > 0
    if kind == "camera":
        assert set(CAMERA_NAMES) <= set(without)
    _same_bits(with_abs, without, f"chain/{kind}")
    for k, v in without.items():
        assert np.abs(v).max() > 0 or k == "dL_dcov3D", k


def test_default_order_keeps_every_other_bit_with_two_addends(gpu):
    """sh_layout_scenes' deg3 under one part of dL_masks at a time: a row gets at most two non-zero
    addends, so the atomics' order cannot show, and the absolute sums are exact as well: the
    default order's are the deterministic order's bit for bit."""
    sc = L.get("deg3")
    reached = 0
    for part, mask in enumerate(L.dL_masks()):
        dL = np.ascontiguousarray(sc["dL"] * mask)
        with_abs = _call(sc, gpu, dL)
        _same_bits(with_abs, _call(sc, gpu, dL, absgrad=False), f"part {part}")
        ordered = _call(sc, gpu, dL, det=True)
        _same_bits(with_abs, ordered, f"part {part}, against the deterministic order")
        reached += (with_abs["dL_dmeans2D_abs"][:, :2] > 0).any(axis=1)
    assert (reached > 0).sum() >= 40 and (reached > 1).sum() >= 10


# ---- 4 --------------------------------------------------------------------------------------------
def test_one_lit_pixel_is_the_signed_gradient(gpu):
    sc = grad_scenes.get("chain")
    hit = 0
    for y, x in ((10, 17), (23, 39), (0, 0)):  # mid-frame, the partial corner quadrant, the origin
        dL = np.zeros_like(sc["dL"])
        dL[:, y, x] = sc["dL"][:, y, x]
        for det in (True, False):  # (one addend per row: exact in both orders)
            g = _call(sc, gpu, dL, det=det)
            np.testing.assert_array_equal(_bits(g["dL_dmeans2D_abs"]),
                                          _bits(np.abs(g["dL_dmeans2D"])), err_msg=f"{y},{x}")
        hit += int((g["dL_dmeans2D_abs"][:, :2] > 0).any(axis=1).sum())
    assert hit >= 3


@pytest.mark.parametrize("loss", ("colour", "combined"))
def test_negated_gradients_give_the_same_bits(loss, gpu):
    sc = grad_scenes.get("long_lists" if loss == "colour" else "chain")
    dL, dLp = ab.loss_gradients(sc, loss)
    a = _call(sc, gpu, dL, dLp, det=True)
    b = _call(sc, gpu, -dL, None if dLp is None else -dLp, det=True)
    np.testing.assert_array_equal(_bits(a["dL_dmeans2D_abs"]), _bits(b["dL_dmeans2D_abs"]))
    np.testing.assert_array_equal(a["dL_dmeans2D"], -b["dL_dmeans2D"])  # (every sum is odd)
    assert np.abs(a["dL_dmeans2D_abs"]).max() > 0


def test_reproducible(gpu):
    sc, other = grad_scenes.get("long_lists"), grad_scenes.get("chain")
    first = _call(sc, gpu, sc["dL"], det=True)
    _same_bits(_call(sc, gpu, sc["dL"], det=True), first, "a second call")
    side = torch.cuda.Stream(gpu)
    with torch.cuda.stream(side):
        again = _call(sc, gpu, sc["dL"], det=True, stream=side.cuda_stream)
    _same_bits(again, first, "a second stream")
    run_hip(other["s"], gpu, colors_precomp=other["colors"], cov3D_precomp=other["cov6"])
    _call(other, gpu, other["dL"])
    _call(other, gpu, other["dL"], pg.plane_dL("chain"), det=True)
    _same_bits(_call(sc, gpu, sc["dL"], det=True), first, "after another frame")
    _same_bits(_call(sc, gpu, sc["dL"], det=True, slot=OTHER_SLOT), first, "another context")


# ---- 5 --------------------------------------------------------------------------------------------
@ORDERS
def test_cancellation(det, gpu):
    """One isotropic Gaussian on a tile's centre under an even image gradient: the signed gradient
    cancels, the absolute one does not.  (The ratio is a condition on the scene, which
    test_absgrad_reference.py checks of the reference.)"""
    sc = ab.cancellation_scene()
    g = _call(sc, gpu, sc["dL"], det=det)
    a, s = g["dL_dmeans2D_abs"][0, :2], np.abs(g["dL_dmeans2D"][0, :2])
    print(f"|dL_dmeans2D| = {s}, dL_dmeans2D_abs = {a}")
    assert (a > 0).all() and (s <= ab.CANCEL_RATIO * a).all()
    fwd = run_hip(sc["s"], gpu)
    ref = ab.scene_abs_gradients(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"], sc["dL"])
    assert gr.rel_err(g["dL_dmeans2D_abs"], ref["means2D_abs"]) <= ab.bound()


# ---- 6 --------------------------------------------------------------------------------------------
def _strip_case(case):
    """(scene, whole-frame dL, the partition) of a strips case."""
    if case == "chain":
        sc = grad_scenes.get("chain")
        return sc, sc["dL"], ((0, 1), (1, 2))
    sc = fs.get("frame")
    dL = fs.masked(sc, planes=False)[0]
    return sc, dL, ss.STRIPS["frame"] if case == "frame3" else ((0, 4), (4, 9))


def _without_a_tile(fwd, sc, strip):
    """[P] bool: the Gaussian is on no list of the strip's tiles (upstream's lists)."""
    gx = (sc["W"] + 15) // 16
    ranges = np.asarray(fwd["ranges"]).reshape(-1, 2).astype(np.int64)
    listed = np.zeros(len(sc["s"]["g"].xyz), bool)
    for tile in range(strip[0] * gx, strip[1] * gx):
        listed[fwd["point_list"][ranges[tile, 0]:ranges[tile, 1]].astype(np.int64)] = True
    return ~listed


@ORDERS
@pytest.mark.parametrize("case", ("chain", "frame2", "frame3"))
def test_strips_add_up_to_the_frame(case, det, gpu):
    """Each strip's and the frame's output lie within the row bound b of their references, which
    are non-negative and add up exactly, so |sum of strips - frame| <= b (sum + frame) word by
    word, up to the second order in b."""
    sc, dL, strips = _strip_case(case)
    fwd = _forward(sc, gpu) if case == "chain" else _fwd(sc, gpu)
    frame = _call(sc, gpu, dL, det=det)["dL_dmeans2D_abs"].astype(np.float64)
    total, none_seen = np.zeros_like(frame), 0
    for strip in strips:
        y0, y1 = ss.pixel_rows(sc, strip)
        got = _call(sc, gpu, np.ascontiguousarray(dL[:, y0:y1]), det=det, strip=strip)
        none = _without_a_tile(fwd, sc, strip)
        none_seen += int(none.sum())
        assert _bits(got["dL_dmeans2D_abs"][none]).max(initial=0) == 0  # +0.0 in all three words
        assert (got["dL_dmeans2D_abs"] >= 0).all()
        total += got["dL_dmeans2D_abs"].astype(np.float64)
    assert none_seen >= 1 and np.abs(frame).max() > 0
    b = ab.row_bound()
    slack = b * (1 + b) * (total + frame) + np.finfo(np.float32).tiny
    worst_word = float((np.abs(total - frame) / slack).max())
    print(f"{case}: |sum of strips - frame| at most {worst_word:.3f} of its allowance")
    assert (np.abs(total - frame) <= slack).all()
    assert ((total == 0) == (frame == 0)).all()


@pytest.mark.parametrize("case", ("chain", "frame2"))
def test_the_whole_frame_as_a_strip_has_the_frames_bits(case, gpu):
    sc, dL, _ = _strip_case(case)
    gy = (sc["H"] + 15) // 16
    frame = _call(sc, gpu, dL, det=True)
    _same_bits(_call(sc, gpu, dL, det=True, strip=(0, gy)), frame, f"{case} (0, {gy})")
    by_ext = _ext(sc, gpu, dL, True, strip=(0, gy))
    np.testing.assert_array_equal(_bits(by_ext[11].cpu().numpy()),
                                  _bits(frame["dL_dmeans2D_abs"]))


# ---- 7 --------------------------------------------------------------------------------------------
SENTINEL = -559038737  # 0xDEADBEEF as int32


def _raw(sc, gpu, out_ptr, P=None, det=True):
    """gsr_backward_abs through the C ABI with dL_dmeans2D_abs at out_ptr; the return code."""
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
                                bg=held[3].data_ptr())
    dLd = to_dev(sc["dL"], gpu)
    means3D = torch.zeros((len(s["g"].xyz), 3), device=gpu)
    rc = _lib.backward_abs_fn(lib)(
        _lib.context(gpu.index or 0, 0), ctypes.byref(g), ctypes.byref(st),
        ctypes.byref(_lib.GsrBackwardInputs(dL_dcolor=dLd.data_ptr())), None, None, None,
        ctypes.byref(_lib.GsrBackwardOrder(deterministic=int(det))), None,
        ctypes.byref(_lib.GsrAbsGradients(dL_dmeans2D_abs=out_ptr)),
        ctypes.byref(_lib.GsrGradients(dL_dmeans3D=means3D.data_ptr())),
        ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    torch.cuda.synchronize(gpu)
    return rc


def test_guard_words_around_an_unaligned_output(gpu):
    sc = grad_scenes.get("chain")
    P = len(sc["s"]["g"].xyz)
    want = _call(sc, gpu, sc["dL"], det=True)["dL_dmeans2D_abs"]
    buf = torch.full((3 * P + 9,), SENTINEL, dtype=torch.int32, device=gpu)
    out = buf[5:5 + 3 * P]
    assert out.data_ptr() % 16 == 4
    assert _raw(sc, gpu, out.data_ptr()) == 0
    host = buf.cpu().numpy()
    assert (host[:5] == SENTINEL).all() and (host[5 + 3 * P:] == SENTINEL).all()
    np.testing.assert_array_equal(host[5:5 + 3 * P].view(np.uint32), _bits(want).reshape(-1))


def test_no_gaussian_writes_nothing(gpu):
    sc = grad_scenes.get("chain")
    buf = torch.full((64,), SENTINEL, dtype=torch.int32, device=gpu)
    for det in (False, True):
        assert _raw(sc, gpu, buf.data_ptr(), P=0, det=det) == 0  # GSR_OK
        assert (buf.cpu().numpy() == SENTINEL).all()


# ---- 8 --------------------------------------------------------------------------------------------
def test_grad_accumulates_over_backward_calls(gpu):
    sc = grad_scenes.get("chain")
    d = _inputs(sc, gpu)
    P = len(sc["s"]["g"].xyz)
    raster = GaussianRasterizer(_settings(sc, gpu, deterministic=True))
    dLs = (to_dev(sc["dL"], gpu), to_dev(pg.plane_dL("chain"), gpu))

    def run(leaf, abs_leaf, dL):
        d["means3D"].requires_grad_(True)
        color, _ = raster(means2D=leaf, means2D_abs=abs_leaf, **d)
        (color * dL).sum().backward()

    singles = []
    for dL in dLs:
        leaf, abs_leaf = (torch.zeros((P, 3), device=gpu, requires_grad=True) for _ in range(2))
        run(leaf, abs_leaf, dL)
        singles.append((leaf.grad.clone(), abs_leaf.grad.clone()))
    leaf, abs_leaf = (torch.zeros((P, 3), device=gpu, requires_grad=True) for _ in range(2))
    for dL in dLs:
        run(leaf, abs_leaf, dL)
    assert torch.equal(abs_leaf.grad, singles[0][1] + singles[1][1])
    assert torch.equal(leaf.grad, singles[0][0] + singles[1][0])
    assert float(abs_leaf.grad.max()) > 0 and abs_leaf.grad.shape == (P, 3)


def test_argument_checks(gpu):
    sc = grad_scenes.get("chain")
    d = _inputs(sc, gpu)
    P = len(sc["s"]["g"].xyz)
    raster = GaussianRasterizer(_settings(sc, gpu))
    ok = lambda **kw: torch.zeros((P, 3), **{"device": gpu, "requires_grad": True, **kw})  # noqa: E731
    with pytest.raises(RuntimeError, match="means2D_abs with features"):
        raster(means2D=None, means2D_abs=ok(), features=torch.zeros((P, 4), device=gpu), **d)
    bad = (torch.zeros((P, 2), device=gpu, requires_grad=True),
           torch.zeros((P + 1, 3), device=gpu, requires_grad=True),
           ok(dtype=torch.float64), ok(device="cpu"), ok(requires_grad=False),
           np.zeros((P, 3), np.float32))
    for t in bad:
        with pytest.raises(ValueError, match="means2D_abs"):
            raster(means2D=None, means2D_abs=t, **d)
    # a shading renders, and raises at backward like every backward
    d["means3D"].requires_grad_(True)
    shaded = GaussianRasterizer(_settings(sc, gpu, shading=_lib.GSR_SHADE_BILLBOARD))
    color, _ = shaded(means2D=None, means2D_abs=ok(), **d)
    with pytest.raises(RuntimeError, match="no backward under shading"):
        color.sum().backward()


def test_composes_with_the_other_options(gpu):
    """depth_maps, a camera gradient, antialiasing, a strip and torch's global switch at once: the
    ctypes call's bits in means2D_abs.grad, and every other .grad is the call's without the leaf."""
    sc = grad_scenes.get("chain")
    strip = (1, 2)
    y0, y1 = ss.pixel_rows(sc, strip)
    dL = np.ascontiguousarray(sc["dL"][:, y0:y1])
    dLp = np.ascontiguousarray(pg.plane_dL("chain")[:, y0:y1])

    def run(absgrad):
        d = _inputs(sc, gpu)
        for v in d.values():
            if v is not None:
                v.requires_grad_(True)
        P = len(sc["s"]["g"].xyz)
        view = to_dev(sc["s"]["view"], gpu).requires_grad_(True)
        leaves = dict(d, view=view, means2D=torch.zeros((P, 3), device=gpu, requires_grad=True))
        kw = {}
        if absgrad:
            leaves["means2D_abs"] = kw["means2D_abs"] = torch.zeros((P, 3), device=gpu,
                                                                    requires_grad=True)
        rs = _settings(sc, gpu, view=view, depth_maps=True, antialiasing=True, tile_rows=strip)
        out = GaussianRasterizer(rs)(means2D=leaves["means2D"], **d, **kw)
        assert len(out) == 5 and out[0].shape == (3, y1 - y0, sc["W"])
        loss = (out[0] * to_dev(dL, gpu)).sum()
        for i in range(3):
            loss = loss + (out[2 + i] * to_dev(dLp[i], gpu)).sum()
        loss.backward()
        return {k: t.grad.cpu().numpy() for k, t in leaves.items() if t is not None}

    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        with_abs, without = run(True), run(False)
    finally:
        torch.use_deterministic_algorithms(was)
    _same_bits(with_abs, without, "GaussianRasterizer, every option")
    by_ctypes = _call(sc, gpu, dL, dLp, det=True, strip=strip, camera=True, aa=True)
    np.testing.assert_array_equal(_bits(with_abs["means2D_abs"]),
                                  _bits(by_ctypes["dL_dmeans2D_abs"]))
    np.testing.assert_array_equal(_bits(with_abs["view"]).reshape(-1),
                                  _bits(by_ctypes["dL_dviewmatrix"]).reshape(-1))
    assert np.abs(with_abs["means2D_abs"]).max() > 0


def test_report_worst():
    """Not a check: prints the largest error seen per (scene, loss) as a share of its bound."""
    for key, (e, e_row) in sorted(worst.items()):
        print(f"{key}: per tensor {e:.3f} of the bound, per row {e_row:.3f} of the bound")
