"""The gradients of per-Gaussian feature channels (gsr_backward_features) on the
device, against autograd of the float64 restatement (feature_grad_reference) on the scenes of
grad_scenes.

Per gradient tensor e = max|g_gpu - g_ref64| / max|g_ref64| must stay within 8 x f, f the
reference's own float32 spread under these losses (feature_grad_reference.F32_SPREAD, measured on
the CPU).  The reference's integer decisions (lists, radii) are the GPU forward's exported state;
its float gates are float64's, and no scene has a decision within rounding of a gate
(test_feature_grad_reference.py).

  1 features alone (dL_dcolor NULL) and colour plus features, C in 1, 5, 17, on the four scenes:
    dL_dfeatures, the 2D gradients, every input leaf
  2 S1, everything at once: planes, camera, antialiasing, features
  3 exact zeros in dL_dfeatures for culled Gaussians and, on a strip, for Gaussians without a tile
    in it; guard words around [P, C]
  4 the two S1 strips' gradients add up to the frame's
  5 deterministic = 1 is refused and nothing is written
  6 GaussianRasterizer(..., features=f)
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import camera_grad_reference as cgr
import feature_grad_reference as fg
import grad_reference as gr
import grad_scenes
import plane_grad_reference as pg
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer, _scene_structs,
                                                    rasterize_gaussians_backward_native)
from gpu_helpers import run_hip, to_dev
from test_gpu_backward import END_TO_END, _forward, _inputs

pytestmark = pytest.mark.gpu

_ref_cache = {}
_worst = {}


def _reference(sc, gpu, loss, C):
    """Autograd of the float64 restatement on the GPU forward's lists and radii."""
    key = (sc["name"], loss, C)
    if key not in _ref_cache:
        fwd = _forward(sc, gpu)
        ref = fg.scene_gradients(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"],
                                 *fg.loss_gradients(sc, loss, C))
        assert ref["near"] == (0, 0, 0)
        _ref_cache[key] = ref
    return _ref_cache[key]


def _backward(sc, gpu, dL, feat, dLf, **kw):
    """gsr_backward_features by ctypes; dL None travels as NULL."""
    s, d = sc["s"], _inputs(sc, gpu)
    g = rasterize_gaussians_backward_native(
        to_dev(s["bg"], gpu), d["means3D"], d["colors_precomp"], d["opacities"], d["scales"],
        d["rotations"], s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], to_dev(dL, gpu), d["shs"], s["sh_degree"],
        to_dev(s["campos"], gpu), features=to_dev(feat, gpu), dL_dfeature_map=to_dev(dLf, gpu),
        **kw)
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items()}


def _close(got, ref, key, what, table=None):
    e = fg.err(got, ref, key)
    b = fg.bound(key, table)
    size = ref["S"][key] if key in cgr.CAMERA else np.abs(ref[key]).max()
    print(f"{what}: e[{key}] = {e:.3e}  (bound {b:.1e}, {e / b:.3f} of it, size {size:.3e})")
    _worst[key] = max(_worst.get(key, 0.0), e / b)
    return [] if e <= b else [f"{what}: e[{key}] = {e:.3e} > {b:.1e}"]


def _check_all(got, ref, sc, what, table=None, two_d=True):
    bad = _close(got["dL_dfeatures"], ref, "features", what, table)
    if two_d:
        px = got["dL_dmeans2D"][:, :2] / np.array([0.5 * sc["W"], 0.5 * sc["H"]])
        bad += _close(px, ref, "means2D_px", what)
        bad += _close(got["dL_dconic"], ref, "conic", what)
    for name, key in END_TO_END:
        if key in ref and name in got and (table is None or key in table):
            if key in ("colors", "shs") and np.abs(ref[key]).max() == 0:
                assert (got[name] == 0).all(), f"{what}: {name} from features"
                continue
            bad += _close(got[name], ref, key, what, table)
    assert not bad, bad
    assert (got["dL_dmeans2D"][:, 2] == 0).all()


@pytest.mark.parametrize("C", fg.CHANNELS)
@pytest.mark.parametrize("loss", fg.LOSSES)
@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_gradients(name, loss, C, gpu):
    """Check 1.  Under the features' loss alone dL_dcolor is NULL, no colour pass runs, and
    dL_dcolors and dL_dsh stay exact zeros."""
    sc = grad_scenes.get(name)
    ref = _reference(sc, gpu, loss, C)
    got = _backward(sc, gpu, *fg.loss_gradients(sc, loss, C), conic=True)
    assert got["dL_dfeatures"].shape == (len(sc["s"]["g"].xyz), C)
    _check_all(got, ref, sc, f"{name}/{loss}/C={C}")
    if loss == "features":
        assert (got["dL_dcolors"] == 0).all()
    culled = _forward(sc, gpu)["radii"] == 0
    assert (got["dL_dfeatures"][culled] == 0).all()


def test_everything_at_once(gpu):
    """Check 2 (S1): colour, the three planes, the camera's gradients, the antialiased forward and
    ALL_C feature channels in one call, each tensor on the scale of its own measured spread."""
    sc = grad_scenes.get(fg.ALL_SCENE)
    fwd = _forward(sc, gpu)
    ref = fg.all_gradients(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"])
    assert ref["near"] == (0, 0, 0)
    dLp = pg.plane_dL(sc["name"])
    got = _backward(sc, gpu, sc["dL"], fg.feature_rows(sc["name"], fg.ALL_C),
                    fg.feature_dL(sc["name"], fg.ALL_C), camera=True, antialiasing=True,
                    **{f"dL_d{n}": to_dev(dLp[i], gpu) for i, n in enumerate(pg.PLANES)})
    _check_all(got, ref, sc, "everything", fg.F32_SPREAD_ALL, two_d=False)
    bad = []
    for name in cgr.CAMERA:
        bad += _close(got[f"dL_d{name}"], ref, name, "everything", fg.F32_SPREAD_ALL)
    assert not bad, bad


def _raw_backward(sc, gpu, feat, dLf, d_feat, deterministic=0, dL=None, tile_rows=(0, 0)):
    """gsr_backward_features with a caller-owned dL_dfeatures pointer; returns (rc, gradients)."""
    s, d = sc["s"], _inputs(sc, gpu)
    _, _, P, g, st, held = _scene_structs(
        to_dev(s["bg"], gpu), d["means3D"], d["colors_precomp"], d["opacities"], d["scales"],
        d["rotations"], s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], sc["H"], sc["W"], d["shs"], s["sh_degree"],
        to_dev(s["campos"], gpu), False, False)
    st.tile_row_begin, st.tile_row_end = tile_rows
    grads = {n: torch.full(shape, 7.0, device=gpu) for n, shape in
             (("dL_dmeans3D", (P, 3)), ("dL_dmeans2D", (P, 3)), ("dL_dopacity", (P, 1)))}
    out = _lib.GsrGradients(**{n: t.data_ptr() for n, t in grads.items()})
    feat_t, dLf_t, dL_t = to_dev(feat, gpu), to_dev(dLf, gpu), to_dev(dL, gpu)
    fgr = _lib.GsrFeatureGradients(C=feat.shape[1], features=feat_t.data_ptr(),
                                   dL_dfeature_map=dLf_t.data_ptr(), dL_dfeatures=d_feat)
    lib = _lib.load_library()
    rc = _lib.features_fns(lib)[1](
        _lib.context(gpu.index or 0, 0), ctypes.byref(g), ctypes.byref(st),
        ctypes.byref(_lib.GsrBackwardInputs(dL_dcolor=_lib.ptr(dL_t))), None, None, None,
        ctypes.byref(_lib.GsrBackwardOrder(deterministic=deterministic)), ctypes.byref(fgr),
        ctypes.byref(out), ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    torch.cuda.synchronize(gpu)
    return rc, grads


@pytest.mark.parametrize("C", (5, 17))
def test_guard_words_and_zeroing(C, gpu):
    """Check 3 (S4): the words before and after [P, C] stay untouched; the buffer is zeroed, then
    filled -- a poisoned one ends with the gradients of a clean call, exact zeros for the culled."""
    sc = grad_scenes.get("edges")
    P = len(sc["s"]["g"].xyz)
    feat, dLf = fg.feature_rows("edges", C), fg.feature_dL("edges", C)
    buf = torch.full((8 + P * C + 8,), 1234.5, device=gpu)
    rc, _ = _raw_backward(sc, gpu, feat, dLf, buf.data_ptr() + 32)
    assert rc == 0
    assert (buf[:8] == 1234.5).all() and (buf[-8:] == 1234.5).all()
    got = buf[8:-8].view(P, C).cpu().numpy().astype(np.float64)
    ref = _reference(sc, gpu, "features", C)
    bad = _close(got, ref, "features", f"edges/poisoned/C={C}")
    assert not bad, bad
    culled = _forward(sc, gpu)["radii"] == 0
    assert culled.sum() >= 5 and (got[culled] == 0).all() and (np.signbit(got[culled]) == 0).all()
    # dL_dfeatures NULL: only the geometry's gradients, the same as with it
    rc, geo = _raw_backward(sc, gpu, feat, dLf, None)
    assert rc == 0
    rc, geo2 = _raw_backward(sc, gpu, feat, dLf, buf.data_ptr() + 32)
    for n in geo:
        e = gr.rel_err(geo[n].cpu().numpy(), geo2[n].cpu().numpy())
        assert e <= fg.bound("means2D" if n == "dL_dmeans2D" else n[4:]), (n, e)


def _strip_gradients(sc, gpu, strip, loss, C):
    dL, feat, dLf = fg.loss_gradients(sc, loss, C)
    y0, y1 = 16 * strip[0], min(sc["H"], 16 * strip[1])
    return _backward(sc, gpu, None if dL is None else dL[:, y0:y1], feat, dLf[:, y0:y1],
                     tile_rows=strip, image_height=sc["H"], conic=True)


@pytest.mark.parametrize("loss", fg.LOSSES)
def test_strips_add_up_to_the_frame(loss, gpu):
    """Checks 3 and 4 (S1, strips (0, 1) and (1, 2), C = 17): a Gaussian without a tile in the
    strip gets exact zeros; the strips' gradients add up to the frame's."""
    sc = grad_scenes.get("chain")
    C = 17
    ref = _reference(sc, gpu, loss, C)
    total = None
    for strip in ((0, 1), (1, 2)):
        got = _strip_gradients(sc, gpu, strip, loss, C)
        touched = run_hip(sc["s"], gpu, tile_rows=strip, extras=("tiles_touched",),
                          binning=False)["tiles_touched"]
        outside = touched == 0
        assert 0 < outside.sum() < len(outside)
        assert (got["dL_dfeatures"][outside] == 0).all()
        assert (got["dL_dmeans3D"][outside] == 0).all()
        assert np.abs(got["dL_dfeatures"][~outside]).max() > 0
        total = got if total is None else {k: total[k] + got[k] for k in got}
    _check_all(total, ref, sc, f"chain/strips/{loss}")
    frame = _backward(sc, gpu, *fg.loss_gradients(sc, loss, C), conic=True)
    for name, key in (("dL_dfeatures", "features"),) + END_TO_END:
        if name in frame and np.abs(frame[name]).max() > 0:
            e = gr.rel_err(total[name], frame[name])
            print(f"strips vs frame: e[{key}] = {e:.3e}")
            assert e <= fg.bound(key), (name, e)


def test_deterministic_is_refused_and_writes_nothing(gpu):
    """Check 5: order->deterministic == 1 with a feature gradient: GSR_E_INVALID, the message says
    why, and no gradient buffer is touched."""
    sc = grad_scenes.get("chain")
    P, C = len(sc["s"]["g"].xyz), 5
    buf = torch.full((P * C,), 1234.5, device=gpu)
    rc, grads = _raw_backward(sc, gpu, fg.feature_rows("chain", C), fg.feature_dL("chain", C),
                              buf.data_ptr(), deterministic=1, dL=sc["dL"])
    msg = _lib.load_library().gsr_last_error()
    assert rc == -1 and b"deterministic" in msg and b"no room" in msg
    assert (buf == 1234.5).all() and all((t == 7.0).all() for t in grads.values())
    with pytest.raises(RuntimeError, match="deterministic"):
        _backward(sc, gpu, sc["dL"], fg.feature_rows("chain", C), fg.feature_dL("chain", C),
                  deterministic=True)
    # ... and without a feature gradient the deterministic mode is what it was
    rc, grads = _raw_backward(sc, gpu, fg.feature_rows("chain", C), fg.feature_dL("chain", C),
                              None, deterministic=1, dL=sc["dL"])
    assert rc == -1  # (a map is given: still refused, dL_dfeatures or not)


def _settings(sc, gpu, **kw):
    s = sc["s"]
    return GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu),
        False, False, **kw)


def _module(sc, gpu, feat, dL, dLf, **kw):
    """Gradients through GaussianRasterizer(..., features=f) of sum(color * dL) +
    sum(feature_map * dLf) (dL None: the features' loss alone), by their gsr_gradients names."""
    d = _inputs(sc, gpu)
    for v in d.values():
        if v is not None:
            v.requires_grad_(True)
    f = to_dev(feat, gpu).requires_grad_(True)
    means2D = torch.zeros_like(d["means3D"], requires_grad=True)
    out = GaussianRasterizer(_settings(sc, gpu, **kw))(means2D=means2D, features=f, **d)
    assert len(out) == 3 and not out[1].requires_grad and out[0].requires_grad
    assert out[2].requires_grad and tuple(out[2].shape) == tuple(dLf.shape)
    loss = (out[2] * to_dev(dLf, gpu)).sum()
    if dL is not None:
        loss = loss + (out[0] * to_dev(dL, gpu)).sum()
    loss.backward()
    grad = lambda t: None if t is None or t.grad is None else t.grad.cpu().numpy().astype(np.float64)  # noqa: E731
    got = dict(dL_dfeatures=grad(f), dL_dmeans3D=grad(d["means3D"]), dL_dmeans2D=grad(means2D),
               dL_dopacity=grad(d["opacities"]), dL_dscales=grad(d["scales"]),
               dL_drotations=grad(d["rotations"]), dL_dsh=grad(d["shs"]),
               dL_dcov3D=grad(d["cov3D_precomp"]), dL_dcolors=grad(d["colors_precomp"]))
    return {k: v for k, v in got.items() if v is not None}


@pytest.mark.parametrize("loss", fg.LOSSES)
@pytest.mark.parametrize("name", ("chain", "precomputed"))
def test_rasterizer_module(name, loss, gpu):
    """Check 6: f.grad and every leaf's gradient match the reference within the bound and the
    native call within the bound; a call without features returns today's tuple."""
    sc = grad_scenes.get(name)
    C = 5
    dL, feat, dLf = fg.loss_gradients(sc, loss, C)
    ref = _reference(sc, gpu, loss, C)
    got = _module(sc, gpu, feat, dL, dLf)
    _check_all(got, ref, sc, f"{name}/module/{loss}", two_d=False)
    native = _backward(sc, gpu, dL, feat, dLf)
    assert gr.rel_err(got["dL_dfeatures"], native["dL_dfeatures"]) <= fg.bound("features")
    d = _inputs(sc, gpu)
    d["means3D"].requires_grad_(True)
    plain = GaussianRasterizer(_settings(sc, gpu))(means2D=None, **d)
    assert len(plain) == 2 and type(plain[0].grad_fn).__name__ == "_RasterizeGaussiansBackward"
    deep = GaussianRasterizer(_settings(sc, gpu, depth_maps=True))(means2D=None, **d)
    assert len(deep) == 5 and type(deep[0].grad_fn).__name__ == "_RasterizeGaussiansPlanesBackward"


def test_rasterizer_module_composes(gpu):
    """S1 through the module with depth_maps, antialiasing and a camera that requires gradients:
    the everything-at-once reference; and the two strips' f.grad add up to the frame's."""
    sc = grad_scenes.get(fg.ALL_SCENE)
    fwd = _forward(sc, gpu)
    ref = fg.all_gradients(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"])
    s, d = sc["s"], _inputs(sc, gpu)
    for k in ("means3D", "opacities", "scales", "rotations", "shs"):
        d[k].requires_grad_(True)
    f = to_dev(fg.feature_rows(sc["name"], fg.ALL_C), gpu).requires_grad_(True)
    cam = [to_dev(s[k], gpu).requires_grad_(True) for k in ("view", "proj", "campos")]
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"], cam[0],
        cam[1], s["sh_degree"], cam[2], False, False, depth_maps=True, antialiasing=True)
    out = GaussianRasterizer(rs)(means2D=None, features=f, **d)
    assert len(out) == 6
    dLp = pg.plane_dL(sc["name"])
    loss = (out[0] * to_dev(sc["dL"], gpu)).sum() + \
        (out[5] * to_dev(fg.feature_dL(sc["name"], fg.ALL_C), gpu)).sum()
    for i in range(3):
        loss = loss + (out[2 + i] * to_dev(dLp[i], gpu)).sum()
    loss.backward()
    g64 = lambda t: t.grad.cpu().numpy().astype(np.float64)  # noqa: E731
    bad = _close(g64(f), ref, "features", "module/everything", fg.F32_SPREAD_ALL)
    for t, key in ((d["means3D"], "means3D"), (d["opacities"], "opacity"), (d["scales"], "scales"),
                   (d["rotations"], "rotations"), (d["shs"], "shs"), (cam[0], "viewmatrix"),
                   (cam[1], "projmatrix"), (cam[2], "campos")):
        n = ref[key].size  # (campos may travel as a homogeneous 4-vector)
        bad += _close(g64(t).reshape(-1)[:n], ref, key, "module/everything", fg.F32_SPREAD_ALL)
    assert not bad, bad
    # tile_rows: each strip's f.grad; their sum is the frame's
    C = 5
    feat, dLf = fg.feature_rows("chain", C), fg.feature_dL("chain", C)
    total = 0.0
    for strip in ((0, 1), (1, 2)):
        y0, y1 = 16 * strip[0], min(sc["H"], 16 * strip[1])
        total = total + _module(sc, gpu, feat, None, dLf[:, y0:y1], tile_rows=strip)["dL_dfeatures"]
    bad = _close(total, _reference(sc, gpu, "features", C), "features", "module/strips")
    assert not bad, bad


def test_rasterizer_module_determinism(gpu):
    """deterministic=True with features raises at backward; deterministic=None under
    torch.use_deterministic_algorithms(True) raises likewise, and with warn_only=True warns and runs
    the atomic path; deterministic=False runs it silently."""
    sc = grad_scenes.get("chain")
    C = 5
    dL, feat, dLf = fg.loss_gradients(sc, "combined", C)
    ref = _reference(sc, gpu, "combined", C)
    with pytest.raises(RuntimeError, match="deterministic"):
        _module(sc, gpu, feat, dL, dLf, deterministic=True)
    was, was_warn = (torch.are_deterministic_algorithms_enabled(),
                     torch.is_deterministic_algorithms_warn_only_enabled())
    try:
        torch.use_deterministic_algorithms(True)
        with pytest.raises(RuntimeError, match="deterministic"):
            _module(sc, gpu, feat, dL, dLf)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*float atomics.*")
            got = _module(sc, gpu, feat, dL, dLf, deterministic=False)
        torch.use_deterministic_algorithms(True, warn_only=True)
        with pytest.warns(UserWarning, match="float atomics"):
            warned = _module(sc, gpu, feat, dL, dLf)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
    for g in (got, warned):
        bad = _close(g["dL_dfeatures"], ref, "features", "chain/module/determinism")
        assert not bad, bad


def test_report_worst_fraction():
    """The largest error of this file's checks as a fraction of its bound, per tensor (printed for
    the README's table; runs last)."""
    print({k: f"{v:.3f}" for k, v in sorted(_worst.items())})
    assert all(v <= 1.0 for v in _worst.values())
