"""The backward pass (gsr_backward and its planes, camera and antialiasing forms) on
the device at frame scale, against float64 autograd on the scenes of frame_grad_scenes: many waves
adding to one gradient row, quadrants wholly outside the image, waves that stop before the end of
their list, the per-pair binning form (more than 256 tile columns, more than 256 tile rows with
pixel y up to 4111), the rebuild's depth sort forms,
scratch buffers that shrink and grow again, the camera's sums over many live blocks.

Per gradient tensor e = max|g_gpu - g_ref64| / max|g_ref64| (the camera's three: cam_err) must
stay within 8 x f, f the reference's own float32 spread on the same scene and loss
(frame_grad_scenes.F32_SPREAD, measured on the CPU).  The reference's integers are the C oracle's
lists and radii, which the GPU forward's exported state must equal (asserted first); the image
gradients are zero at every pixel with a decision within frame_grad_scenes.BAND of a gate, so such
a pixel adds nothing whichever way the device decides.

  1 the three checks of test_gpu_backward.py (blend alone, per-Gaussian alone, end to end by
    ctypes; by `_C` on frame) on frame, wall, wide and tall
  2 an image gradient in one 8 x 8 quadrant: exact zeros for every Gaussian outside that tile's
    list, the others within the bound relative to that quadrant's own largest gradient (tall: in
    the first, a middle and the last tile row)
  3 wall: exact zeros from the blend for the Gaussians no pixel composites
  4 frame with planes, camera and antialiasing at once, then without antialiasing
  5 frame, colour + planes, under every depth sort form, without the blend cull, without the
    second stream
  6 one context through frame, chain, frame with the camera, wide, chain
"""
import numpy as np
import pytest
import torch

import frame_grad_scenes as fs
import grad_reference as gr
import grad_scenes
import plane_grad_reference as pg
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer,
                                                    rasterize_gaussians_backward_native)
from gpu_helpers import set_option, to_dev
from test_gpu_backward import END_TO_END, _assert_end_to_end, _forward, _inputs
from test_gpu_backward import _reference as _toy_reference

pytestmark = pytest.mark.gpu

CAMERA = (("dL_dviewmatrix", "viewmatrix"), ("dL_dprojmatrix", "projmatrix"), ("dL_dcampos", "campos"))
BLEND = (("dL_dconic", "conic"), ("dL_dcolors", "rgb"))
worst = {}  # the largest e / bound seen per (loss, tensor) (printed by the last test)
# (context slots of this file alone; test_gpu_antialiasing.py hands out 300 upwards)
OPTION_SLOT = 400
_next_slot = [400]


def _new_slot():
    _next_slot[0] += 1
    return _next_slot[0]


def _fwd(sc, gpu):
    """The GPU forward with every extra, its lists and radii equal to the oracle's (the CPU-side
    mask and the references rely on that) and its records the oracle's bits."""
    fwd = _forward(sc, gpu)
    if "checked" not in fwd:
        orc = fs.oracle_of(sc)
        for k in ("radii", "ranges", "point_list"):
            np.testing.assert_array_equal(fwd[k], orc[k], err_msg=k)
        for k in ("means2D", "conic_opacity", "rgb"):
            np.testing.assert_array_equal(fwd[k].view(np.uint32), orc[k].view(np.uint32), err_msg=k)
        fwd["checked"] = True
    return fwd


def _backward(sc, gpu, dL, dLp=None, camera=False, aa=False, conic=False, slot=0, colors=None):
    s, d = sc["s"], _inputs(sc if colors is None else dict(sc, colors=colors), gpu)
    kw = {} if dLp is None else {f"dL_d{n}": to_dev(dLp[i], gpu) for i, n in enumerate(pg.PLANES)}
    g = rasterize_gaussians_backward_native(
        to_dev(s["bg"], gpu), d["means3D"], d["colors_precomp"], d["opacities"], d["scales"],
        d["rotations"], s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], to_dev(dL, gpu), d["shs"],
        s["sh_degree"] if colors is None else 0, to_dev(s["campos"], gpu), conic=conic,
        camera=camera, antialiasing=aa, slot=slot, **kw)
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items()}


def _px(got, sc):
    return got["dL_dmeans2D"][:, :2] / np.array([0.5 * sc["W"], 0.5 * sc["H"]])


def _close(got, ref, key, name, kind, what):
    """The failures of one tensor against ref[key] within the bound of (scene, loss)."""
    e, b = fs.err(got, ref, key), fs.bound(name, kind, key)
    worst[(kind, key)] = max(worst.get((kind, key), 0.0), e / b)
    print(f"{what}: e[{key}] = {e:.3e} = {e / b:.3f} of the bound {b:.1e}")
    return [] if e <= b else [f"{what}: e[{key}] = {e:.3e} > {b:.1e}"]


def _all_close(got, ref, name, kind, what, pairs=END_TO_END):
    bad, seen = [], 0
    for out, key in pairs:
        if key in ref and out in got and key in fs.F32_SPREAD[(name, kind)]:
            bad += _close(got[out], ref, key, name, kind, what)
            seen += 1
    assert seen >= 6 and not bad, bad


# ---- 1 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fs.NAMES)
def test_blend_backward_alone(name, gpu):
    """The GPU forward's own means2D, conic_opacity and rgb as leaves of composite."""
    sc = fs.get(name)
    fwd = _fwd(sc, gpu)
    dL, _ = fs.masked(sc, planes=False)
    got = _backward(sc, gpu, dL, conic=True)
    leaf = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64), requires_grad=True)  # noqa: E731
    m2, conic = leaf(fwd["means2D"]), leaf(fwd["conic_opacity"][:, :3])
    op, rgb = leaf(fwd["conic_opacity"][:, 3]), leaf(fwd["rgb"])
    color, _, _ = gr.composite((fwd["ranges"], fwd["point_list"]), m2, conic, op, rgb,
                               sc["s"]["bg"], sc["W"], sc["H"])
    (color * torch.tensor(dL.astype(np.float64))).sum().backward()
    ref = dict(means2D_px=m2.grad.numpy(), conic=conic.grad.numpy(), opacity=op.grad.numpy(),
               rgb=rgb.grad.numpy())
    bad = _close(_px(got, sc), ref, "means2D_px", name, "colour", name)
    bad += _close(got["dL_dconic"], ref, "conic", name, "colour", name)
    bad += _close(got["dL_dopacity"].reshape(-1), ref, "opacity", name, "colour", name)
    bad += _close(got["dL_dcolors"], ref, "rgb", name, "colour", name)
    assert not bad, bad
    assert (got["dL_dmeans2D"][:, 2] == 0).all()


@pytest.mark.parametrize("name", fs.NAMES)
def test_per_gaussian_backward_alone(name, gpu):
    """torch.autograd.grad of project with the GPU's 2D gradients as grad_outputs."""
    sc = fs.get(name)
    fwd = _fwd(sc, gpu)
    got = _backward(sc, gpu, fs.masked(sc, planes=False)[0], conic=True)
    lv = gr.leaves(sc, torch.float64)
    m2, conic, rgb, _, near = gr.project(gr.camera_constants(sc["s"]), fwd["radii"], lv["means3D"],
                                         lv["means2D"], lv["scales"], lv["rotations"], None,
                                         lv["shs"])
    assert near == 0
    keys = ("means3D", "scales", "rotations", "shs")
    grads = torch.autograd.grad([m2, conic, rgb], [lv[k] for k in keys],
                                [torch.tensor(_px(got, sc)), torch.tensor(got["dL_dconic"]),
                                 torch.tensor(got["dL_dcolors"])])
    names = dict(means3D="dL_dmeans3D", scales="dL_dscales", rotations="dL_drotations", shs="dL_dsh")
    bad = []
    for k, g in zip(keys, grads):
        bad += _close(got[names[k]], {k: g.numpy()}, k, name, "colour", name)
    assert not bad, bad


@pytest.mark.parametrize("name,path", [(n, "ctypes") for n in fs.NAMES] + [("frame", "C")])
def test_end_to_end(name, path, gpu):
    """Every gradient against composite(project(...)), by ctypes and (frame) through autograd of
    GaussianRasterizer (the `_C` extension)."""
    sc = fs.get(name)
    _fwd(sc, gpu)
    ref = fs.reference(sc, "colour")
    dL, _ = fs.masked(sc, planes=False)
    if path == "ctypes":
        got = _backward(sc, gpu, dL)
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
        (color * to_dev(dL, gpu)).sum().backward()
        grad = lambda t: t.grad.cpu().numpy().astype(np.float64)  # noqa: E731
        got = dict(dL_dmeans3D=grad(d["means3D"]), dL_dmeans2D=grad(means2D),
                   dL_dopacity=grad(d["opacities"]), dL_dscales=grad(d["scales"]),
                   dL_drotations=grad(d["rotations"]), dL_dsh=grad(d["shs"]))
    _all_close(got, ref, name, "colour", f"{name}/{path}")
    assert (got["dL_dmeans2D"][:, 2] == 0).all()
    culled = fs.oracle_of(sc)["radii"] == 0
    for k, v in got.items():
        assert (v[culled] == 0).all(), k


# ---- 2 --------------------------------------------------------------------------------------------
def _is_zero(v):
    """Every value is +0.0 or -0.0, by its float32 bits (the per-Gaussian stage multiplies a zero
    row by signed factors)."""
    bits = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return bool(((bits & np.uint32(0x7FFFFFFF)) == 0).all())


@pytest.mark.parametrize("name,tile_x,tile_y,quad", fs.PLACEMENTS)
def test_localised_image_gradient(name, tile_x, tile_y, quad, gpu):
    """dL non-zero in one 8 x 8 quadrant only: every gradient of every Gaussian outside that
    tile's list is zero bit for bit (a sum sent to the wrong row shows here), the others are within
    the bound of the reference, now relative to that quadrant's own largest gradient."""
    sc = fs.get(name)
    fwd = _fwd(sc, gpu)
    dL = fs.localized(sc, tile_x, tile_y, quad)
    got = _backward(sc, gpu, dL, conic=True)
    tile = tile_y * ((sc["W"] + 15) // 16) + tile_x
    r0, r1 = (int(v) for v in fwd["ranges"][tile])
    listed = np.zeros(len(sc["s"]["g"].xyz), bool)
    listed[fwd["point_list"][r0:r1].astype(np.int64)] = True
    assert 0 < listed.sum() < len(listed)
    for k, v in got.items():
        assert _is_zero(v[~listed]), k
    assert np.abs(got["dL_dmeans3D"][listed]).max() > 0
    ref = fs.localized_reference(sc, tile_x, tile_y, quad)
    what = f"{name} tile ({tile_x}, {tile_y}) quadrant {quad}"
    bad = _close(_px(got, sc), ref, "means2D_px", name, "local", what)
    assert not bad, bad
    _all_close(got, ref, name, "local", what, END_TO_END + BLEND)


# ---- 3 --------------------------------------------------------------------------------------------
def test_wall_uncomposited_get_exact_zeros(gpu):
    """wall: the Gaussians no pixel composites (hidden behind the layer where every wave has
    stopped, or too faint) get zeros from the blend bit for bit -- dL_dconic, and dL_dcolors with
    precomputed colours, which is the blend's own sum -- while the composited ones of the near
    layer do not."""
    sc = fs.get("wall")
    fwd = _fwd(sc, gpu)
    comp = fs.composited(sc)
    assert (~comp).sum() >= 100
    dL, _ = fs.masked(sc, planes=False)
    got = _backward(sc, gpu, dL, conic=True, colors=fwd["rgb"])
    assert "dL_dsh" not in got
    front = sc["special"]["front"][comp[sc["special"]["front"]]]
    for k in ("dL_dconic", "dL_dcolors"):
        assert _is_zero(got[k][~comp]), k
        assert (np.abs(got[k][front]).max(axis=1) > 0).all(), k
    # and with the colours precomputed the blend's sums are the SH run's
    ref = fs.reference(sc, "colour")
    bad = _close(got["dL_dconic"], ref, "conic", "wall", "colour", "wall/precomputed")
    bad += _close(got["dL_dcolors"], ref, "rgb", "wall", "colour", "wall/precomputed")
    assert not bad, bad


# ---- 4 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", (True, False))
def test_frame_with_every_extension(aa, gpu):
    """frame with dL_ddepth_map, dL_dinv_depth_map and dL_dfinal_T all set and camera=True,
    antialiased (k_blend_bwd_planes_q and k_preprocess_bwd_planes_camera_aa) against
    aa_reference.scene_gradients, then plain against camera_grad_reference.scene_gradients."""
    sc = fs.get("frame")
    _fwd(sc, gpu)
    kind = "all_aa" if aa else "all"
    ref = fs.reference(sc, kind)
    dL, dLp = fs.masked(sc)
    got = _backward(sc, gpu, dL, dLp, camera=True, aa=aa)
    got["dL_dcampos"] = got["dL_dcampos"].reshape(-1)[:3]
    _all_close(got, ref, "frame", kind, f"frame/{kind}", END_TO_END + CAMERA)
    assert all(n in got for n, _ in CAMERA)


# ---- 5 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,value", [(_lib.GSR_OPT_DEPTH_SORT, v) for v in (0, 1, 2, 3)] +
                         [(_lib.GSR_OPT_BLEND_CULL, 0), (_lib.GSR_OPT_SECOND_STREAM, 0)],
                         ids=["depth_sort_0", "depth_sort_1", "depth_sort_2", "depth_sort_3",
                              "blend_cull_0", "second_stream_0"])
def test_frame_under_options(opt, value, gpu):
    """frame, colour + planes, under each form of the rebuild's depth sort (the planes' backward
    gathers z from the sort's keys by Gaussian id, whichever form ran), without the blend cull and
    without the second stream; the option reads back unchanged after the backward."""
    sc = fs.get("frame")
    _fwd(sc, gpu)
    ref = fs.reference(sc, "all")
    dL, dLp = fs.masked(sc)
    ctx = _lib.context(gpu.index or 0, OPTION_SLOT)
    before = _lib.get_option(ctx, opt)
    set_option(gpu, opt, value, OPTION_SLOT)
    try:
        got = _backward(sc, gpu, dL, dLp, slot=OPTION_SLOT)
        assert _lib.get_option(ctx, opt) == value
    finally:
        set_option(gpu, opt, before, OPTION_SLOT)
    assert _lib.get_option(ctx, opt) == before
    _all_close(got, ref, "frame", "all", f"frame, option {opt} = {value}")


# ---- 6 --------------------------------------------------------------------------------------------
def test_buffer_reuse_on_one_context(gpu):
    """One fresh context through frame (P = 6,000), chain (96), frame with the camera, wide
    (3,000), chain: the gradient rows, the rebuild's radii and the camera's partials shrink and
    grow again between the calls; each result against its own reference."""
    slot = _new_slot()
    frame, wide, chain = fs.get("frame"), fs.get("wide"), grad_scenes.get("chain")
    for sc in (frame, wide):
        _fwd(sc, gpu)
    ref_chain = _toy_reference(chain, gpu)
    dL, dLp = fs.masked(frame)
    _all_close(_backward(frame, gpu, dL, slot=slot), fs.reference(frame, "colour"), "frame",
               "colour", "1 frame")
    toy = lambda: {k: v.cpu().numpy().astype(np.float64) for k, v in  # noqa: E731
                   rasterize_gaussians_backward_native(
                       to_dev(chain["s"]["bg"], gpu), *_toy_args(chain, gpu), slot=slot).items()}
    _assert_end_to_end(toy(), ref_chain, "2 chain")
    got = _backward(frame, gpu, dL, dLp, camera=True, slot=slot)
    got["dL_dcampos"] = got["dL_dcampos"].reshape(-1)[:3]
    _all_close(got, fs.reference(frame, "all"), "frame", "all", "3 frame, camera",
               END_TO_END + CAMERA)
    _all_close(_backward(wide, gpu, fs.masked(wide, planes=False)[0], slot=slot),
               fs.reference(wide, "colour"), "wide", "colour", "4 wide")
    _assert_end_to_end(toy(), ref_chain, "5 chain")


def _toy_args(sc, gpu):
    """The arguments of the native backward after bg for a grad_scenes scene, as
    test_gpu_backward._backward passes them."""
    s, d = sc["s"], _inputs(sc, gpu)
    return (d["means3D"], d["colors_precomp"], d["opacities"], d["scales"], d["rotations"],
            s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu), to_dev(s["proj"], gpu),
            s["tx"], s["ty"], to_dev(sc["dL"], gpu), d["shs"], s["sh_degree"],
            to_dev(s["campos"], gpu))


def test_report_worst_ratio():
    """Not a check of its own: prints the largest e / bound the tests above saw per loss and tensor
    (DESIGN.md 3e quotes it)."""
    for (kind, key), v in sorted(worst.items()):
        print(f"{kind:8s} {key:12s} {v:.3f}")
