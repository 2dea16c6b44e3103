"""GPU: every word of every gradient row of the backward against its own float64 bound
(row_grad_reference; DESIGN.md 4, "Every gradient row against its own bound").

Every other backward test reduces a tensor to max|got - ref| / max|ref|, which lets a row five
decades under the tensor's maximum be anything.  Here a word may differ from the float64 reference
by 8 x ROW_SPREAD x S, S the sum of the absolute values of what is added to that word (for a 3D
word: carried through the row's own Jacobian of the per-Gaussian stage), and is exactly 0.0 where S
is: culled Gaussians, Gaussians no pixel composites, SH coefficients above the active degree.  No
row is left out; the frame scenes keep their pixel masks.

Scenes: chain, long_lists, precomputed, edges (grad_scenes), wall and frame (frame_grad_scenes,
masked), long_lists@oblique (pose_scenes).  The references' integer decisions (lists, radii) are the
GPU forward's exported state; their float gates are float64's.

  1 the blend stage alone: dL_dmeans2D (in pixels), dL_dconic, dL_dopacity, dL_dcolors -- and with
    planes dL_ddepths -- against the closed-form sums on the forward's own float32 records
  2 end to end, colour and colour + the three planes, by ctypes, through GaussianRasterizer (`_C`)
    and with deterministic = 1
"""
import numpy as np
import pytest
import torch

import frame_grad_scenes as fs
import grad_reference as gr
import plane_grad_reference as pg
import row_grad_reference as rr
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer)
from gpu_helpers import to_dev
from test_gpu_backward import END_TO_END, _forward, _inputs
from test_gpu_backward_frames import _fwd
from test_gpu_deterministic_backward import _call

pytestmark = pytest.mark.gpu

LOSSES = ("colour", "planes")
_cache = {}
worst = {}  # (scene, loss, what, key) -> row_err / bound (printed by the last test)


def _scene(name, gpu):
    """(sc, dL, dLp, fwd): the GPU forward's lists are the oracle's on the frame scenes, whose
    masks were decided on those."""
    sc, dL, dLp = rr.case(name)
    return sc, dL, dLp, (_fwd(sc, gpu) if name in fs.NAMES else _forward(sc, gpu))


def _end_to_end_reference(name, loss, gpu):
    """(ref, sums, S) on the GPU forward's lists and radii, once per scene and loss."""
    key = ("e2e", name, loss)
    if key not in _cache:
        sc, dL, dLp, fwd = _scene(name, gpu)
        _cache[key] = rr.scene_scales(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"], dL,
                                      dLp if loss == "planes" else None)
        if name not in fs.NAMES:
            assert _cache[key][0]["near"] == (0, 0)
    return _cache[key]


def _blend_reference(name, loss, gpu):
    """The closed-form sums of the blend on the forward's own float32 records, under the float64
    gates of those records."""
    key = ("blend", name, loss)
    if key not in _cache:
        sc, dL, dLp, fwd = _scene(name, gpu)
        t = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64))  # noqa: E731
        feat = fwd["rgb"] if sc["colors"] is None else sc["colors"]
        rec = (t(fwd["means2D"]), t(fwd["conic_opacity"][:, :3]), t(fwd["conic_opacity"][:, 3]),
               t(feat))
        lists = (fwd["ranges"], fwd["point_list"])
        with torch.no_grad():
            _, gates, near = gr.composite(lists, *rec, sc["s"]["bg"], sc["W"], sc["H"])
        if name not in fs.NAMES:
            assert near == 0
        _cache[key] = rr.blend_sums(lists, rec, gates, sc["W"], sc["H"], sc["s"]["bg"], dL,
                                    dLp if loss == "planes" else None,
                                    fwd["depths"].astype(np.float64))
    return _cache[key]


def _where(name, gpu, S, row):
    """Where a row's largest addends come from: its tile and list position there."""
    sc, _, _, fwd = _scene(name, gpu)
    tile, pos = int(S["tile"][row]), int(S["pos"][row])
    gx = (sc["W"] + 15) // 16
    n = int(fwd["ranges"][tile][1]) - int(fwd["ranges"][tile][0]) if tile >= 0 else 0
    return f"Gaussian {row}: list position {pos} of {n} in tile {tile} = ({tile % gx}, {tile // gx})"


def _hold(name, loss, what, gpu, got, ref, S, pairs):
    """Every (got, key) pair per word under 8 x ROW_SPREAD x S, exact zeros where S == 0."""
    bad, seen = [], 0
    for v, key in pairs:
        e, i, zeros = rr.row_err(v, ref[key], S[key])
        b = rr.bound(key)
        worst[(name, loss, what, key)] = e / b
        print(f"{name}/{loss}/{what}: row_err[{key}] = {e:.3e} = {e / b:.3f} of the bound {b:.1e}"
              f"{'' if zeros else '; non-zero where S == 0'}")
        if not e <= b:
            bad.append(f"{key}: {e:.3e} > {b:.1e} at {i}: {_where(name, gpu, S, int(i[0]))}; got "
                       f"{np.asarray(v).reshape(ref[key].shape)[i]:.6e}, ref {ref[key][i]:.6e}, "
                       f"S {np.asarray(S[key]).reshape(ref[key].shape)[i]:.3e}")
        if not zeros:
            off = (np.asarray(S[key]).reshape(ref[key].shape) == 0) & \
                (np.asarray(v).reshape(ref[key].shape) != 0)
            row = int(np.argwhere(off)[0][0])
            bad.append(f"{key}: {int(off.sum())} non-zero words where S == 0, first in "
                       f"{_where(name, gpu, S, row)}")
        seen += 1
    assert not bad, bad
    return seen


# ---- 1 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", rr.SCENES)
def test_blend_stage_alone(name, loss, gpu):
    sc, dL, dLp, _ = _scene(name, gpu)
    ref = _blend_reference(name, loss, gpu)
    got = _call(sc, gpu, dL, dLp if loss == "planes" else None, det=False, conic=True)
    got = {k: v.astype(np.float64) for k, v in got.items()}
    assert (got["dL_dmeans2D"][:, 2] == 0).all()
    px = got["dL_dmeans2D"][:, :2] / np.array([0.5 * sc["W"], 0.5 * sc["H"]])
    pairs = [(px, "means2D_px"), (got["dL_dconic"], "conic"), (got["dL_dopacity"], "opacity"),
             (got["dL_dcolors"], "rgb")]
    if loss == "planes":
        pairs.append((got["dL_ddepths"], "depths"))
    S = dict(ref["S"], tile=ref["tile"], pos=ref["pos"])
    assert _hold(name, loss, "blend", gpu, got, ref["sum"], S, pairs) == len(pairs)


# ---- 2 --------------------------------------------------------------------------------------------
def _through_autograd(sc, gpu, dL, dLp):
    """The gradients GaussianRasterizer's autograd leaves in its inputs (the `_C` extension), by
    their gsr_gradients names."""
    s, d = sc["s"], _inputs(sc, gpu)
    for v in d.values():
        if v is not None:
            v.requires_grad_(True)
    means2D = torch.zeros_like(d["means3D"], requires_grad=True)
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu),
        False, False, depth_maps=dLp is not None)
    out = GaussianRasterizer(rs)(means2D=means2D, **d)
    loss = (out[0] * to_dev(dL, gpu)).sum()
    if dLp is not None:
        assert len(out) == 5
        for i in range(3):
            loss = loss + (out[2 + i] * to_dev(dLp[i], gpu)).sum()
    loss.backward()
    grad = lambda t: None if t is None else t.grad.cpu().numpy().astype(np.float64)  # noqa: E731
    got = dict(dL_dmeans3D=grad(d["means3D"]), dL_dmeans2D=grad(means2D),
               dL_dopacity=grad(d["opacities"]), dL_dscales=grad(d["scales"]),
               dL_drotations=grad(d["rotations"]), dL_dsh=grad(d["shs"]),
               dL_dcov3D=grad(d["cov3D_precomp"]), dL_dcolors=grad(d["colors_precomp"]))
    return {k: v for k, v in got.items() if v is not None}


@pytest.mark.parametrize("route", ("ctypes", "C", "deterministic"))
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", rr.SCENES)
def test_end_to_end(name, loss, route, gpu):
    sc, dL, dLp, _ = _scene(name, gpu)
    ref, _, S = _end_to_end_reference(name, loss, gpu)
    p = dLp if loss == "planes" else None
    if route == "C":
        got = _through_autograd(sc, gpu, dL, p)
    else:
        got = _call(sc, gpu, dL, p, det=route == "deterministic", conic=False)
        got = {k: v.astype(np.float64) for k, v in got.items()}
    pairs = [(got[out], key) for out, key in END_TO_END
             if key in ref and out in got and (key != "cov3D" or sc["cov6"] is not None)]
    if "dL_ddepths" in got and loss == "planes":
        pairs.append((got["dL_ddepths"], "depths"))
    seen = _hold(name, loss, route, gpu, got, ref, S, pairs)
    assert seen >= (5 if sc["cov6"] is not None else 6)


def test_report_worst_ratio():
    """Not a check of its own: prints row_err / bound per scene, loss, route and tensor (DESIGN.md
    4 quotes the largest per scene and tensor)."""
    for (name, loss, what, key), v in sorted(worst.items()):
        print(f"worst {name:18s} {loss:6s} {what:13s} {key:11s} {v:.3f}")
    assert all(v <= 1.0 for v in worst.values())
