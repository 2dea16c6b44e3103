"""The backward pass (gsr_backward) on the device, against autograd of the float64
restatement of the forward (grad_reference) on the scenes of grad_scenes.

Per gradient tensor e = max|g_gpu - g_ref64| / max|g_ref64| must stay within 8 x f, f the
reference's own float32 spread (grad_reference.F32_SPREAD, measured on the CPU).  The integer
decisions of the reference (lists, radii) are the GPU forward's exported state; its float gates are
float64's, and no scene has a decision within rounding of a gate (test_grad_reference.py).

  1 the blend's backward alone      (composite with the GPU forward's own records as leaves)
  2 the per-Gaussian backward alone (project with the GPU's 2D gradients as grad_outputs)
  3 end to end through autograd, by the `_C` extension and by ctypes
  4 statelessness: interleaved forwards, a repeated backward, every context option, and the
    forward's bits before and after a backward
  5 errors: a strip, a shading; no backward without requires_grad inputs
"""
import ctypes

import numpy as np
import pytest
import torch

import grad_reference as gr
import grad_scenes
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer, binning_state,
                                                    rasterize_gaussians_backward_native)
from gpu_helpers import ALL_EXTRAS, run_hip, set_option, to_dev

pytestmark = pytest.mark.gpu

_fwd_cache, _ref_cache = {}, {}


def _inputs(sc, gpu):
    """The scene's tensors on the device, by GaussianRasterizer's argument names."""
    g, P = sc["s"]["g"], len(sc["s"]["g"].xyz)
    d = dict(means3D=to_dev(g.xyz, gpu), opacities=to_dev(g.opacity, gpu), shs=None,
             colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None)
    if sc["colors"] is None:
        d["shs"] = to_dev(g.sh.reshape(P, -1, 3), gpu)
    else:
        d["colors_precomp"] = to_dev(sc["colors"], gpu)
    if sc["cov6"] is None:
        d["scales"], d["rotations"] = to_dev(g.scale, gpu), to_dev(g.rot, gpu)
    else:
        d["cov3D_precomp"] = to_dev(sc["cov6"], gpu)
    return d


def _forward(sc, gpu, cache=True):
    """The GPU forward with every extra (n_contrib among them: upstream's lists) and its lists."""
    if not cache or sc["name"] not in _fwd_cache:
        out = run_hip(sc["s"], gpu, colors_precomp=sc["colors"], cov3D_precomp=sc["cov6"],
                      extras=ALL_EXTRAS, binning=True)
        if not cache:
            return out
        _fwd_cache[sc["name"]] = out
    return _fwd_cache[sc["name"]]


def _backward(sc, gpu, conic=True):
    s, d = sc["s"], _inputs(sc, gpu)
    g = rasterize_gaussians_backward_native(
        to_dev(s["bg"], gpu), d["means3D"], d["colors_precomp"], d["opacities"], d["scales"],
        d["rotations"], s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], to_dev(sc["dL"], gpu), d["shs"], s["sh_degree"],
        to_dev(s["campos"], gpu), conic=conic)
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items()}


def _reference(sc, gpu):
    """Autograd of composite(project(...)) in float64 on the GPU forward's lists and radii."""
    if sc["name"] not in _ref_cache:
        fwd = _forward(sc, gpu)
        ref = gr.scene_gradients(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"], sc["dL"])
        assert ref["near"] == (0, 0)
        _ref_cache[sc["name"]] = ref
    return _ref_cache[sc["name"]]


def _close(got, ref, key, what):
    e = gr.rel_err(got, ref)
    print(f"{what}: e[{key}] = {e:.3e}  (f = {gr.F32_SPREAD[key]:.1e}, bound {gr.bound(key):.1e}, "
          f"max|ref| = {np.abs(ref).max():.3e})")
    return [] if e <= gr.bound(key) else [f"{what}: e[{key}] = {e:.3e} > {gr.bound(key):.1e}"]


# gsr_gradients member -> (the reference's key, reshape)
END_TO_END = (("dL_dmeans3D", "means3D"), ("dL_dmeans2D", "means2D"), ("dL_dopacity", "opacity"),
              ("dL_dscales", "scales"), ("dL_drotations", "rotations"), ("dL_dsh", "shs"),
              ("dL_dcov3D", "cov3D"), ("dL_dcolors", "colors"))


def _assert_end_to_end(got, ref, what):
    bad = []
    for name, key in END_TO_END:
        if key in ref and name in got:
            bad += _close(got[name].reshape(ref[key].shape), ref[key], key, what)
    assert not bad, bad


@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_blend_backward_alone(name, gpu):
    """Check 1: the GPU forward's own means2D, conic_opacity and rgb as leaves of composite."""
    sc = grad_scenes.get(name)
    fwd, got = _forward(sc, gpu), _backward(sc, gpu)
    feat = fwd["rgb"] if sc["colors"] is None else sc["colors"]
    leaf = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64), requires_grad=True)  # noqa: E731
    m2, conic = leaf(fwd["means2D"]), leaf(fwd["conic_opacity"][:, :3])
    op, rgb = leaf(fwd["conic_opacity"][:, 3]), leaf(feat)
    color, _, near = gr.composite((fwd["ranges"], fwd["point_list"]), m2, conic, op, rgb,
                                  sc["s"]["bg"], sc["W"], sc["H"])
    assert near == 0
    (color * torch.tensor(sc["dL"].astype(np.float64))).sum().backward()
    px = got["dL_dmeans2D"][:, :2] / np.array([0.5 * sc["W"], 0.5 * sc["H"]])
    bad = _close(px, m2.grad.numpy(), "means2D_px", name)
    bad += _close(got["dL_dconic"], conic.grad.numpy(), "conic", name)
    bad += _close(got["dL_dopacity"].reshape(-1), op.grad.numpy(), "opacity", name)
    bad += _close(got["dL_dcolors"], rgb.grad.numpy(), "rgb", name)
    assert not bad, bad
    assert (got["dL_dmeans2D"][:, 2] == 0).all()


@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_per_gaussian_backward_alone(name, gpu):
    """Check 2: torch.autograd.grad of project with the GPU's 2D gradients as grad_outputs."""
    sc = grad_scenes.get(name)
    fwd, got = _forward(sc, gpu), _backward(sc, gpu)
    lv = gr.leaves(sc, torch.float64)
    m2, conic, rgb, _, near = gr.project(gr.camera_constants(sc["s"]), fwd["radii"], lv["means3D"],
                                         lv["means2D"], lv.get("scales"), lv.get("rotations"),
                                         lv.get("cov3D"), lv.get("shs"), lv.get("colors"))
    assert near == 0
    px = got["dL_dmeans2D"][:, :2] / np.array([0.5 * sc["W"], 0.5 * sc["H"]])
    keys = [k for k in ("means3D", "scales", "rotations", "shs", "cov3D") if k in lv]
    grads = torch.autograd.grad([m2, conic, rgb], [lv[k] for k in keys],
                                [torch.tensor(px), torch.tensor(got["dL_dconic"]),
                                 torch.tensor(got["dL_dcolors"])], allow_unused=True)
    names = dict(means3D="dL_dmeans3D", scales="dL_dscales", rotations="dL_drotations",
                 shs="dL_dsh", cov3D="dL_dcov3D")
    bad = []
    for k, g in zip(keys, grads):
        bad += _close(got[names[k]].reshape(g.shape), g.numpy(), k, name)
    assert not bad, bad


@pytest.mark.parametrize("path", ("ctypes", "C"))
@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_end_to_end(name, path, gpu):
    """Check 3: every gradient against composite(project(...)), by ctypes and through autograd of
    GaussianRasterizer (the `_C` extension)."""
    sc = grad_scenes.get(name)
    ref = _reference(sc, gpu)
    if path == "ctypes":
        got = _backward(sc, gpu, conic=False)
    else:
        s, d = sc["s"], _inputs(sc, gpu)
        for v in d.values():
            if v is not None:
                v.requires_grad_(True)
        means2D = torch.zeros_like(d["means3D"], requires_grad=True)
        rs = GaussianRasterizationSettings(
            sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
            to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu),
            False, False)
        color, radii = GaussianRasterizer(rs)(means2D=means2D, **d)
        assert color.requires_grad and not radii.requires_grad
        (color * to_dev(sc["dL"], gpu)).sum().backward()
        assert tuple(means2D.grad.shape) == (len(s["g"].xyz), 3)
        grad = lambda t: None if t is None else t.grad.cpu().numpy().astype(np.float64)  # noqa: E731
        got = dict(dL_dmeans3D=grad(d["means3D"]), dL_dmeans2D=grad(means2D),
                   dL_dopacity=grad(d["opacities"]), dL_dscales=grad(d["scales"]),
                   dL_drotations=grad(d["rotations"]), dL_dsh=grad(d["shs"]),
                   dL_dcov3D=grad(d["cov3D_precomp"]), dL_dcolors=grad(d["colors_precomp"]))
        got = {k: v for k, v in got.items() if v is not None}
    _assert_end_to_end(got, ref, f"{name}/{path}")
    assert (got["dL_dmeans2D"][:, 2] == 0).all()


def test_culled_and_inactive_get_exact_zeros(gpu):
    """S4: every gradient of a Gaussian the forward culls is exactly 0.0, and so is the gradient
    of every SH coefficient above the active degree."""
    sc = grad_scenes.get("edges")
    fwd, got = _forward(sc, gpu), _backward(sc, gpu)
    culled = fwd["radii"] == 0
    sp = sc["special"]
    assert culled[sp["behind"]].all() and culled[sp["det0"]].all() and not culled[sp["clamp"]].any()
    for k, v in got.items():
        assert (v[culled] == 0).all(), k
    n = (sc["s"]["sh_degree"] + 1) ** 2
    assert (got["dL_dsh"][:, n:] == 0).all() and np.abs(got["dL_dsh"][:, :n]).max() > 0
    assert (np.abs(got["dL_dmeans3D"][sp["clamp"]]).max(axis=1) > 0).all()


def test_statelessness(gpu):
    """Check 4: backward A after forward A, forward B; a repeated backward; every context option;
    the lists gsr_get_binning exports afterwards; the forward's bits before and after."""
    a, b = grad_scenes.get("chain"), grad_scenes.get("long_lists")
    ref_a, ref_b = _reference(a, gpu), _reference(b, gpu)
    before = _forward(a, gpu, cache=False)
    _forward(b, gpu, cache=False)
    _assert_end_to_end(_backward(a, gpu), ref_a, "A after forward B")
    pl, _, rg = binning_state(gpu.index or 0)
    np.testing.assert_array_equal(pl.cpu().numpy().view(np.uint32), before["point_list"])
    np.testing.assert_array_equal(rg.cpu().numpy().view(np.uint32), before["ranges"])
    _assert_end_to_end(_backward(b, gpu), ref_b, "B after backward A")
    _assert_end_to_end(_backward(b, gpu), ref_b, "B again")
    ctx = _lib.context(gpu.index or 0)
    for opt, values in ((_lib.GSR_OPT_TIGHT_BINNING, (0, 1)), (_lib.GSR_OPT_BLEND_FAST, (0, 1)),
                        (_lib.GSR_OPT_FRAME_GRAPHS, (1, 0))):
        for v in values:  # (the second value is the default)
            set_option(gpu, opt, v)
            try:
                if opt == _lib.GSR_OPT_FRAME_GRAPHS and v:
                    # recorded graphs stay usable around a backward
                    run_hip(a["s"], gpu, extras=(), binning=False)
                    replayed = run_hip(a["s"], gpu, extras=(), binning=False)
                _assert_end_to_end(_backward(a, gpu), ref_a, f"option {opt} = {v}")
                assert _lib.get_option(ctx, opt) == v
                if opt == _lib.GSR_OPT_FRAME_GRAPHS and v:
                    again = run_hip(a["s"], gpu, extras=(), binning=False)
                    np.testing.assert_array_equal(again["color"].view(np.uint32),
                                                  replayed["color"].view(np.uint32))
                    assert _lib.frame_graph_stats(gpu.index or 0)["graph_frames"] >= 2
            finally:
                set_option(gpu, opt, 1 if opt != _lib.GSR_OPT_FRAME_GRAPHS else 0)
    after = _forward(a, gpu, cache=False)
    for k in ("color", "final_T", "n_contrib", "radii", "point_list", "ranges"):
        np.testing.assert_array_equal(np.ascontiguousarray(after[k]).view(np.uint32),
                                      np.ascontiguousarray(before[k]).view(np.uint32), err_msg=k)


def test_errors(gpu):
    """Check 5: a strip and a shading raise; without requires_grad inputs there is no backward."""
    sc = grad_scenes.get("chain")
    s, d = sc["s"], _inputs(sc, gpu)
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu),
        False, False)
    color, _ = GaussianRasterizer(rs)(means2D=None, **d)
    assert not color.requires_grad and color.grad_fn is None
    d["means3D"].requires_grad_(True)
    color, _ = GaussianRasterizer(rs._replace(shading=_lib.GSR_SHADE_FLAT_BALL))(means2D=None, **d)
    with pytest.raises(RuntimeError, match="splat composite only"):
        color.sum().backward()
    # a strip, through the C ABI (the Python entries have no strip argument)
    lib = _lib.load_library()
    dL = to_dev(sc["dL"], gpu)
    g = _lib.GsrGaussians(P=len(s["g"].xyz), D=3, M=16, scale_modifier=1.0,
                          means3D=d["means3D"].data_ptr(), scales=d["scales"].data_ptr(),
                          rotations=d["rotations"].data_ptr(), opacities=d["opacities"].data_ptr(),
                          shs=d["shs"].data_ptr())
    st = _lib.GsrRasterSettings(image_width=sc["W"], image_height=sc["H"], tanfovx=s["tx"],
                                tanfovy=s["ty"], tile_row_begin=0, tile_row_end=1)
    out = _lib.GsrGradients()
    with pytest.raises(RuntimeError, match="whole frames only"):
        _lib.check(_lib.backward_fn(lib)(_lib.context(gpu.index or 0), ctypes.byref(g),
                                         ctypes.byref(st),
                                         ctypes.byref(_lib.GsrBackwardInputs(dL_dcolor=dL.data_ptr())),
                                         ctypes.byref(out), None), "gsr_backward")
