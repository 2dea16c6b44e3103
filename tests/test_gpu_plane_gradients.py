"""The gradients of depth_map, inv_depth_map and final_T (gsr_backward_planes) on the
device, against autograd of the float64 restatement (plane_grad_reference) on the scenes of
grad_scenes.

Per gradient tensor e = max|g_gpu - g_ref64| / max|g_ref64| must stay within 8 x f, f the
reference's own float32 spread under these losses (plane_grad_reference.F32_SPREAD, measured on the
CPU).  The reference's integer decisions (lists, radii) are the GPU forward's exported state; its
float gates are float64's, and no scene has a decision within rounding of a gate.

  1 the blend's backward alone, planes only (dL_dcolor NULL), dL_ddepths against one z leaf
  2 end to end, colour plus three planes, by ctypes and through GaussianRasterizer(depth_maps=True)
  3 one plane at a time (the others NULL; None gradients through autograd)
  4 the forward identities of the new return
  5 stereo.metric_disparity back-propagates to the inputs
  6 culled Gaussians get exact zeros
  7 statelessness
  8 a NULL struct is gsr_backward
  9 errors
"""
import ctypes

import numpy as np
import pytest
import torch

import grad_reference as gr
import grad_scenes
import plane_grad_reference as pg
from gaussiansplattingviewer_amd import _lib, stereo
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer, binning_state,
                                                    rasterize_gaussians_backward_native,
                                                    rasterize_gaussians_native)
from gpu_helpers import run_hip, to_dev
from test_gpu_backward import END_TO_END, _forward, _inputs

pytestmark = pytest.mark.gpu

_ref_cache = {}


def _reference(sc, gpu, loss):
    """Autograd of the float64 restatement on the GPU forward's lists and radii; loss: a name
    pg.loss_gradients knows."""
    key = (sc["name"], loss)
    if key not in _ref_cache:
        fwd = _forward(sc, gpu)
        ref = pg.scene_gradients(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"],
                                 *pg.loss_gradients(sc, loss))
        assert ref["near"] == (0, 0)
        _ref_cache[key] = ref
    return _ref_cache[key]


def _backward(sc, gpu, loss, conic=False, depths=False):
    """gsr_backward_planes by ctypes under a loss of pg.loss_gradients; a plane the loss does not
    use is passed as NULL, and so is dL_dcolor."""
    s, d = sc["s"], _inputs(sc, gpu)
    dL, dLp = pg.loss_gradients(sc, loss)
    planes = {f"dL_d{n}": to_dev(dLp[i], gpu) for i, n in enumerate(pg.PLANES)
              if loss not in pg.PLANES or n == loss}
    g = rasterize_gaussians_backward_native(
        to_dev(s["bg"], gpu), d["means3D"], d["colors_precomp"], d["opacities"], d["scales"],
        d["rotations"], s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], to_dev(dL, gpu), d["shs"], s["sh_degree"],
        to_dev(s["campos"], gpu), conic=conic, depths=depths, **planes)
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items()}


def _settings(sc, gpu, **kw):
    s = sc["s"]
    return GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu),
        False, False, **kw)


def _autograd(sc, gpu, loss_of, between=None):
    """Gradients of loss_of(color, depth_map, inv_depth_map, final_T) through
    GaussianRasterizer(depth_maps=True), by their gsr_gradients names; between() runs after the
    forward."""
    d = _inputs(sc, gpu)
    for v in d.values():
        if v is not None:
            v.requires_grad_(True)
    means2D = torch.zeros_like(d["means3D"], requires_grad=True)
    out = GaussianRasterizer(_settings(sc, gpu, depth_maps=True))(means2D=means2D, **d)
    assert len(out) == 5 and not out[1].requires_grad
    assert all(out[i].requires_grad for i in (0, 2, 3, 4))
    if between is not None:
        between()
    loss_of(out[0], *out[2:]).backward()
    grad = lambda t: None if t is None else t.grad.cpu().numpy().astype(np.float64)  # noqa: E731
    got = dict(dL_dmeans3D=grad(d["means3D"]), dL_dmeans2D=grad(means2D),
               dL_dopacity=grad(d["opacities"]), dL_dscales=grad(d["scales"]),
               dL_drotations=grad(d["rotations"]), dL_dsh=grad(d["shs"]),
               dL_dcov3D=grad(d["cov3D_precomp"]), dL_dcolors=grad(d["colors_precomp"]))
    return {k: v for k, v in got.items() if v is not None}


def _linear_loss(sc, gpu, loss):
    """The loss of pg.loss_gradients(sc, loss) on the rasterizer's outputs; an output it does not
    use does not enter (its gradient arrives as None)."""
    dL, dLp = pg.loss_gradients(sc, loss)

    def loss_of(color, *planes):
        total = 0.0
        if dL is not None:
            total = total + (color * to_dev(dL, gpu)).sum()
        for i, n in enumerate(pg.PLANES):
            if loss not in pg.PLANES or n == loss:
                total = total + (planes[i] * to_dev(dLp[i], gpu)).sum()
        return total
    return loss_of


def _close(got, ref, key, what, table=None):
    e, b = gr.rel_err(got, ref), pg.bound(key, table)
    print(f"{what}: e[{key}] = {e:.3e}  (bound {b:.1e}, max|ref| = {np.abs(ref).max():.3e})")
    return [] if e <= b else [f"{what}: e[{key}] = {e:.3e} > {b:.1e}"]


def _assert_end_to_end(got, ref, what, table=None, keys=None):
    bad = []
    for name, key in END_TO_END:
        if key in ref and name in got and (keys is None or key in keys):
            bad += _close(got[name].reshape(ref[key].shape), ref[key], key, what, table)
    assert not bad, bad


@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_blend_backward_alone_planes_only(name, gpu):
    """Check 1: the GPU forward's own means2D, conic_opacity and depths as leaves of the planes'
    composite; z and 1 / z are two functions of the one depths leaf.  dL_dcolor is NULL."""
    sc = grad_scenes.get(name)
    fwd, got = _forward(sc, gpu), _backward(sc, gpu, "planes", conic=True, depths=True)
    leaf = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64), requires_grad=True)  # noqa: E731
    m2, conic = leaf(fwd["means2D"]), leaf(fwd["conic_opacity"][:, :3])
    op, z = leaf(fwd["conic_opacity"][:, 3]), leaf(fwd["depths"])
    planes, _, near = pg.planes_of((fwd["ranges"], fwd["point_list"]), m2, conic, op,
                                   pg.features(z, fwd["radii"]), sc["W"], sc["H"])
    assert near == 0
    (planes * torch.tensor(pg.plane_dL(name).astype(np.float64))).sum().backward()
    px = got["dL_dmeans2D"][:, :2] / np.array([0.5 * sc["W"], 0.5 * sc["H"]])
    bad = _close(px, m2.grad.numpy(), "means2D_px", name)
    bad += _close(got["dL_dconic"], conic.grad.numpy(), "conic", name)
    bad += _close(got["dL_dopacity"].reshape(-1), op.grad.numpy(), "opacity", name)
    bad += _close(got["dL_ddepths"], z.grad.numpy(), "depths", name)
    assert not bad, bad
    assert (got["dL_dcolors"] == 0).all() and (got["dL_dmeans2D"][:, 2] == 0).all()
    if "dL_dsh" in got:
        assert (got["dL_dsh"] == 0).all()


@pytest.mark.parametrize("path", ("ctypes", "autograd"))
@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_end_to_end(name, path, gpu):
    """Check 2: colour plus all three planes, every input gradient."""
    sc = grad_scenes.get(name)
    ref = _reference(sc, gpu, "combined")
    if path == "ctypes":
        got = _backward(sc, gpu, "combined", depths=True)
        bad = _close(got["dL_ddepths"], ref["depths"], "depths", f"{name}/{path}")
        assert not bad, bad
    else:
        got = _autograd(sc, gpu, _linear_loss(sc, gpu, "combined"))
    _assert_end_to_end(got, ref, f"{name}/{path}")
    assert (got["dL_dmeans2D"][:, 2] == 0).all()


@pytest.mark.parametrize("path", ("ctypes", "autograd"))
@pytest.mark.parametrize("plane", pg.PLANES)
def test_one_plane_at_a_time(plane, path, gpu):
    """Check 3 (S1): the other two planes and dL_dcolor are NULL; through autograd the loss uses
    the one plane and the other outputs' gradients arrive as None."""
    sc = grad_scenes.get(pg.ONE_PLANE_SCENE)
    ref = _reference(sc, gpu, plane)
    if path == "ctypes":
        got = _backward(sc, gpu, plane, depths=True)
        if plane == "final_T":
            assert (got["dL_ddepths"] == 0).all() and (ref["depths"] == 0).all()
        else:
            bad = _close(got["dL_ddepths"], ref["depths"], "depths", f"{plane}/{path}")
            assert not bad, bad
        assert (got["dL_dcolors"] == 0).all()
    else:
        got = _autograd(sc, gpu, _linear_loss(sc, gpu, plane))
    _assert_end_to_end(got, ref, f"{plane}/{path}")


@pytest.mark.parametrize("name", ("chain", "precomputed"))
def test_forward_identities(name, gpu):
    """Check 4: the planes are the extras of rasterize_gaussians_native bit for bit, color and radii
    the plain GaussianRasterizer's; under no_grad nothing is saved."""
    sc = grad_scenes.get(name)
    s, d = sc["s"], _inputs(sc, gpu)
    res = rasterize_gaussians_native(
        to_dev(s["bg"], gpu), d["means3D"], d["colors_precomp"], d["opacities"], d["scales"],
        d["rotations"], s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], sc["H"], sc["W"], d["shs"], s["sh_degree"],
        to_dev(s["campos"], gpu), False, False, extras=pg.PLANES)
    color0, radii0 = GaussianRasterizer(_settings(sc, gpu))(means2D=None, **d)
    with torch.no_grad():
        out = GaussianRasterizer(_settings(sc, gpu, depth_maps=True))(means2D=None, **d)
    assert len(out) == 5 and all(t.grad_fn is None and not t.requires_grad for t in out)
    bits = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    np.testing.assert_array_equal(bits(out[0]), bits(color0))
    np.testing.assert_array_equal(out[1].cpu().numpy(), radii0.cpu().numpy())
    for t, n in zip(out[2:], pg.PLANES):
        assert tuple(t.shape) == (sc["H"], sc["W"]) and t.dtype == torch.float32
        np.testing.assert_array_equal(bits(t), bits(res.extras[n]), err_msg=n)
    # inputs that do not require a gradient: no graph either
    out = GaussianRasterizer(_settings(sc, gpu, depth_maps=True))(means2D=None, **d)
    assert all(t.grad_fn is None for t in out)
    # with one that does, the same bits and a graph on the four image-like outputs
    d["means3D"].requires_grad_(True)
    out = GaussianRasterizer(_settings(sc, gpu, depth_maps=True))(means2D=None, **d)
    assert [t.grad_fn is not None for t in out] == [True, False, True, True, True]
    for t, n in zip(out[2:], pg.PLANES):
        np.testing.assert_array_equal(bits(t.detach()), bits(res.extras[n]), err_msg=n)


def test_metric_disparity_backpropagates(gpu):
    """Check 5 (S1): stereo.metric_disparity of the rasterizer's planes under a random gradient,
    zero where the covered share is below 1e-3, against the same expression on the float64
    reference planes."""
    sc = grad_scenes.get("chain")
    fwd = _forward(sc, gpu)
    final_T = _reference(sc, gpu, "planes")["planes"][2]
    dLd = pg.disparity_dL("chain", final_T)
    ref = pg.scene_gradients(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"], None, None,
                             loss_fn=pg.disparity_loss(sc, dLd))
    assert ref["near"] == (0, 0)

    def loss_of(color, depth_map, inv_depth_map, final_T):
        d = stereo.metric_disparity(inv_depth_map, final_T, sc["s"]["tx"], sc["W"])
        assert d.requires_grad
        return (d * to_dev(dLd, gpu)).sum()
    got = _autograd(sc, gpu, loss_of)
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dscales"):
        assert np.isfinite(got[k]).all() and np.abs(got[k]).max() > 0, k
    _assert_end_to_end(got, ref, "metric_disparity", pg.F32_SPREAD_DISPARITY,
                       keys=pg.F32_SPREAD_DISPARITY)
    assert (got["dL_dsh"] == 0).all()  # the colour is not in the loss


def test_culled_get_exact_zeros(gpu):
    """Check 6 (S4): every gradient of a Gaussian the forward culls is exactly 0.0, dL_ddepths
    included; the clamped ones that reach the frame get a gradient."""
    sc = grad_scenes.get("edges")
    fwd, got = _forward(sc, gpu), _backward(sc, gpu, "combined", conic=True, depths=True)
    culled = fwd["radii"] == 0
    sp = sc["special"]
    assert culled[sp["behind"]].all() and culled[sp["det0"]].all() and not culled[sp["clamp"]].any()
    assert "dL_ddepths" in got
    for k, v in got.items():
        assert (v[culled] == 0).all(), k
    assert (np.abs(got["dL_ddepths"][sp["clamp"]]) > 0).all()


def test_statelessness(gpu):
    """Check 7: backward A after forward A and forward B, repeated; through autograd with another
    scene's forward between forward and backward; the lists gsr_get_binning exports afterwards."""
    a, b = grad_scenes.get("chain"), grad_scenes.get("long_lists")
    ref_a, ref_b = _reference(a, gpu, "combined"), _reference(b, gpu, "combined")
    before = _forward(a, gpu, cache=False)
    _forward(b, gpu, cache=False)
    _assert_end_to_end(_backward(a, gpu, "combined"), ref_a, "A after forward B")
    pl, _, rg = binning_state(gpu.index or 0)
    np.testing.assert_array_equal(pl.cpu().numpy().view(np.uint32), before["point_list"])
    np.testing.assert_array_equal(rg.cpu().numpy().view(np.uint32), before["ranges"])
    _assert_end_to_end(_backward(b, gpu, "combined"), ref_b, "B after backward A")
    _assert_end_to_end(_backward(b, gpu, "combined"), ref_b, "B again")
    got = _autograd(a, gpu, _linear_loss(a, gpu, "combined"),
                    between=lambda: run_hip(b["s"], gpu, extras=(), binning=False))
    _assert_end_to_end(got, ref_a, "A through autograd, forward B in between")
    after = _forward(a, gpu, cache=False)
    for k in ("color", "final_T", "radii", "point_list", "ranges"):
        np.testing.assert_array_equal(np.ascontiguousarray(after[k]).view(np.uint32),
                                      np.ascontiguousarray(before[k]).view(np.uint32), err_msg=k)


def _raw(sc, gpu, dL=None, planes=None, strip=False):
    """gsr_backward_planes through the C ABI with the structs built here: planes is a
    _lib.GsrPlaneGradients or None (a NULL struct).  Returns (rc, gradients dict)."""
    s, d = sc["s"], _inputs(sc, gpu)
    P = len(s["g"].xyz)
    keep = [to_dev(s[k], gpu) for k in ("view", "proj", "campos", "bg")]
    g = _lib.GsrGaussians(P=P, D=s["sh_degree"], M=16 if d["shs"] is not None else 0,
                          scale_modifier=s["scale_modifier"], means3D=_lib.ptr(d["means3D"]),
                          scales=_lib.ptr(d["scales"]), rotations=_lib.ptr(d["rotations"]),
                          opacities=_lib.ptr(d["opacities"]), shs=_lib.ptr(d["shs"]),
                          colors_precomp=_lib.ptr(d["colors_precomp"]),
                          cov3D_precomp=_lib.ptr(d["cov3D_precomp"]))
    st = _lib.GsrRasterSettings(image_width=sc["W"], image_height=sc["H"], tanfovx=s["tx"],
                                tanfovy=s["ty"], viewmatrix=_lib.ptr(keep[0]),
                                projmatrix=_lib.ptr(keep[1]), campos=_lib.ptr(keep[2]),
                                bg=_lib.ptr(keep[3]), tile_row_begin=0,
                                tile_row_end=1 if strip else 0)
    shapes = dict(dL_dmeans3D=(P, 3), dL_dmeans2D=(P, 3), dL_dopacity=(P, 1), dL_dcolors=(P, 3))
    if d["shs"] is not None:
        shapes["dL_dsh"] = (P, 16, 3)
    if d["scales"] is not None:
        shapes.update(dL_dscales=(P, 3), dL_drotations=(P, 4))
    grads = {n: torch.full(sh, 7.0, device=gpu) for n, sh in shapes.items()}
    out = _lib.GsrGradients(**{n: t.data_ptr() for n, t in grads.items()})
    inp = _lib.GsrBackwardInputs(dL_dcolor=_lib.ptr(dL))
    rc = _lib.backward_planes_fn(_lib.load_library())(
        _lib.context(gpu.index or 0), ctypes.byref(g), ctypes.byref(st), ctypes.byref(inp),
        None if planes is None else ctypes.byref(planes), ctypes.byref(out),
        ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    torch.cuda.synchronize(gpu)
    return rc, {k: v.cpu().numpy().astype(np.float64) for k, v in grads.items()}


def test_null_struct_is_gsr_backward(gpu):
    """Check 8: a NULL struct, and a struct without a plane gradient, stay within the colour bounds
    of grad_reference against the colour reference; dL_ddepths is then zero-filled."""
    sc = grad_scenes.get("chain")
    fwd = _forward(sc, gpu)
    ref = gr.scene_gradients(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"], sc["dL"])
    dL = to_dev(sc["dL"], gpu)
    depths = torch.full((len(fwd["radii"]),), 7.0, device=gpu)
    for what, planes in (("NULL struct", None),
                         ("no plane", _lib.GsrPlaneGradients(dL_ddepths=depths.data_ptr()))):
        rc, got = _raw(sc, gpu, dL, planes)
        assert rc == 0, what
        bad = []
        for name, key in END_TO_END:
            if key in ref and name in got:
                e = gr.rel_err(got[name].reshape(ref[key].shape), ref[key])
                print(f"{what}: e[{key}] = {e:.3e}  (bound {gr.bound(key):.1e})")
                if not e <= gr.bound(key):
                    bad.append((what, key, e))
        assert not bad, bad
    assert (depths == 0).all()


def test_errors(gpu):
    """Check 9: a strip and a call without any gradient give GSR_E_INVALID; depth_maps with a
    shading raises at the forward."""
    sc = grad_scenes.get("chain")
    lib = _lib.load_library()
    plane = to_dev(pg.plane_dL("chain")[0], gpu)
    rc, got = _raw(sc, gpu, None, _lib.GsrPlaneGradients(dL_ddepth_map=plane.data_ptr()),
                   strip=True)
    assert rc == -1 and b"whole frames only" in lib.gsr_last_error()
    assert all((v == 7.0).all() for v in got.values())  # nothing was written
    rc, _ = _raw(sc, gpu, None, _lib.GsrPlaneGradients())
    assert rc == -1 and b"dL_dcolor or a plane gradient is required" in lib.gsr_last_error()
    rc, _ = _raw(sc, gpu, None, None)
    assert rc == -1 and b"dL_dcolor is required" in lib.gsr_last_error()
    d = _inputs(sc, gpu)
    d["means3D"].requires_grad_(True)
    rs = _settings(sc, gpu, shading=_lib.GSR_SHADE_FLAT_BALL, depth_maps=True)
    with pytest.raises(RuntimeError, match="come from the splat composite"):
        GaussianRasterizer(rs)(means2D=None, **d)
    with pytest.raises(RuntimeError, match="dL_dout_color or a plane gradient is required"):
        rasterize_gaussians_backward_native(
            to_dev(sc["s"]["bg"], gpu), d["means3D"].detach(), None, d["opacities"], d["scales"],
            d["rotations"], 1.0, None, to_dev(sc["s"]["view"], gpu), to_dev(sc["s"]["proj"], gpu),
            sc["s"]["tx"], sc["s"]["ty"], None, d["shs"], 3, to_dev(sc["s"]["campos"], gpu))
