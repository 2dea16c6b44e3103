"""GPU: every backward path under a general camera pose ("The backward under a general
pose"), against float64 autograd of the references on the scenes of pose_scenes.

Every other gradient test looks through static_camera, whose view rotation is diagonal: R and R^T
are the same numbers there and six entries of projmatrix are exact zeros, so a backward that swaps
a row index for a column index is bit-identical in all of them.  Here the rotation is dense
(poses yaw, oblique, close), and per gradient tensor e (gr.rel_err; the camera's three: cam_err)
against float64 must stay within pose_scenes.bound: 8 x the larger of the kind's existing float32
spread and the one measured under these poses (test_pose_grad_reference.py).  The references'
integer decisions (lists, radii) are the GPU forward's exported state; their float gates are
float64's, and no scene has a decision within rounding of a gate.

  a colour: gsr_backward and gsr_backward_ordered (deterministic), five scenes; the two modes agree
    within rounding; exact zeros for culled Gaussians
  b colour + three planes: chain, pose_edges
  c the camera's three, colour and combined loss, five scenes; the translation identity among the
    call's own outputs; the Gaussians' own gradients keep their bits with and without the camera
    request (deterministic mode, where bits repeat)
  d planes + camera + antialiasing together: chain
  e features with everything at once: chain
  f two tile-row strips of chain, default and deterministic, added on the host in float64 against
    the whole frame's reference
  g GaussianRasterizer(depth_maps=True) with a pose leaf (quaternion + translation -> 4 x 4 view ->
    camera_tensors) at the oblique pose, against float64 autograd of the same chain
"""
import numpy as np
import pytest
import torch

import camera_grad_reference as cg
import feature_grad_reference as fg
import grad_reference as gr
import plane_grad_reference as pg
import pose_scenes as ps
import strip_grad_scenes as ss
from gaussiansplattingviewer_amd.camera import camera_tensors
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizer,
                                                    rasterize_gaussians_backward_native)
from gpu_helpers import ALL_EXTRAS, run_hip, to_dev
from test_gpu_backward import END_TO_END, _forward, _inputs
from test_gpu_camera_gradients import _settings
from test_gpu_deterministic_backward import _call as _native
from test_gpu_feature_gradients import _backward as _feature_backward

pytestmark = pytest.mark.gpu

CAMERA = tuple((f"dL_d{n}", n) for n in cg.CAMERA)
PAIRS = END_TO_END + CAMERA + (("dL_dconic", "conic"), ("dL_dcolors", "rgb"),
                               ("dL_ddepths", "depths"), ("dL_dfeatures", "features"))
_ref_cache = {}
worst = {}  # (kind, tensor) -> the largest e / bound seen (printed by the last test)


def _reference(kind, sc, gpu, loss="combined"):
    key = (kind, sc["name"], loss)
    if key not in _ref_cache:
        fwd = _forward(sc, gpu)
        ref = ps.reference(kind, sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"], loss=loss)
        assert not any(ref["near"]), ref["near"]
        _ref_cache[key] = ref
    return _ref_cache[key]


def _f64(got):
    return {k: np.asarray(v, np.float64) for k, v in got.items()}


def _check(kind, got, ref, sc, what, keys=None):
    """Every tensor of `got` the reference has, under the kind's bound; returns what was seen."""
    got = _f64(got)
    if "dL_dmeans2D" in got:
        assert (got["dL_dmeans2D"][:, 2] == 0).all()
        got["means2D_px"] = got["dL_dmeans2D"][:, :2] / np.array([0.5 * sc["W"], 0.5 * sc["H"]])
    bad, seen = [], []
    for name, key in PAIRS + (("means2D_px", "means2D_px"),):
        if name not in got or key not in ref or key not in ps.POSE_F32_SPREAD[kind] or \
                (keys is not None and key not in keys):
            continue
        v = got[name].reshape(-1)[:ref[key].size] if key in cg.CAMERA else got[name]
        e, b = ps.err(v, ref, key), ps.bound(kind, key)
        worst[(kind, key)] = max(worst.get((kind, key), 0.0), e / b)
        print(f"{what}: e[{key}] = {e:.3e} = {e / b:.3f} of the bound {b:.1e}")
        if not e <= b:
            bad.append(f"{what}: e[{key}] = {e:.3e} > {b:.1e}")
        seen.append(key)
    assert not bad, bad
    return seen


# ---- a --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pose", ps.CASES)
def test_colour(name, pose, gpu):
    sc = ps.get(name, pose)
    ref = _reference("colour", sc, gpu)
    default = _native(sc, gpu, sc["dL"], det=False)
    ordered = _native(sc, gpu, sc["dL"], det=True)
    for got, mode in ((default, "default"), (ordered, "deterministic")):
        seen = _check("colour", got, ref, sc, f"{sc['name']}/{mode}")
        assert len(seen) >= 7 and "means3D" in seen and "conic" in seen
    for out, key in END_TO_END:  # the two modes: the same sums, grouped differently
        if out in default and key in ref and np.abs(ref[key]).max() > 0:
            e = gr.rel_err(default[out].reshape(ref[key].shape), ordered[out].reshape(ref[key].shape))
            assert e <= ps.bound("colour", key), (out, e)
    culled = _forward(sc, gpu)["radii"] == 0
    for k, v in default.items():
        assert (v[culled] == 0).all(), k
    if name == "pose_edges":
        sp = sc["special"]
        assert culled[sp["behind"]].all() and not culled[sp["clamp"]].any()
        assert (np.abs(default["dL_dmeans3D"][sp["clamp"]]).max(axis=1) > 0).all()


# ---- b --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", ps.NAMES)
@pytest.mark.parametrize("name", ps.PLANE_SCENES)
def test_planes(name, pose, gpu):
    sc = ps.get(name, pose)
    got = _native(sc, gpu, sc["dL"], ps.plane_dL(sc), det=False)
    seen = _check("planes", got, _reference("planes", sc, gpu), sc, f"{sc['name']}/planes")
    assert len(seen) >= 8 and "depths" in seen


# ---- c --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ps.CAMERA_LOSSES)
@pytest.mark.parametrize("name,pose", ps.CASES)
def test_camera(name, pose, loss, gpu):
    sc = ps.get(name, pose)
    s = sc["s"]
    ref = _reference("camera", sc, gpu, loss)
    dLp = ps.plane_dL(sc) if loss == "combined" else None
    got = _f64(_native(sc, gpu, sc["dL"], dLp, camera=True, det=False))
    seen = _check("camera", got, ref, sc, f"{sc['name']}/camera/{loss}", cg.CAMERA)
    assert set(seen) == set(cg.CAMERA)
    assert (np.abs(got["dL_dcampos"]).max() > 0) == (sc["colors"] is None)
    dvm, dpm = got["dL_dviewmatrix"].reshape(-1), got["dL_dprojmatrix"].reshape(-1)
    assert (dvm[3::4] == 0).all() and (dpm[2::4] == 0).all()  # the forward never reads them
    # moving every Gaussian is moving the camera the other way (test_translation_identity)
    vm, pm = (np.asarray(s[k], np.float64).reshape(-1) for k in ("view", "proj"))
    bnd = max(ps.bound("camera", n) for n in cg.CAMERA)
    for c in range(3):
        lhs = got["dL_dmeans3D"][:, c].sum()
        rhs = (pm[4 * c:4 * c + 4] * dpm[12:16]).sum() + (vm[4 * c:4 * c + 4] * dvm[12:16]).sum() \
            - got["dL_dcampos"].reshape(-1)[c]
        scale = np.abs(got["dL_dmeans3D"][:, c]).sum()
        print(f"{sc['name']}/{loss}/{c}: |lhs - rhs| / scale = {abs(lhs - rhs) / scale:.3e}")
        assert abs(lhs - rhs) <= bnd * scale
    # the camera's kernels leave the Gaussians' own gradients their bits
    with_cam = _native(sc, gpu, sc["dL"], dLp, camera=True, det=True)
    without = _native(sc, gpu, sc["dL"], dLp, camera=False, det=True)
    for k, v in without.items():
        np.testing.assert_array_equal(v.view(np.uint32), with_cam[k].view(np.uint32), err_msg=k)


# ---- d --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", ps.NAMES)
def test_planes_camera_antialiasing(pose, gpu):
    sc = ps.get(ps.ALL_SCENE, pose)
    got = _native(sc, gpu, sc["dL"], ps.plane_dL(sc), camera=True, aa=True, det=False)
    seen = _check("aa", got, _reference("aa", sc, gpu), sc, f"{sc['name']}/aa")
    assert set(seen) == set(ps.POSE_F32_SPREAD["aa"])


# ---- e --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", ps.NAMES)
def test_features_with_everything(pose, gpu):
    sc = ps.get(ps.ALL_SCENE, pose)
    dLp = ps.plane_dL(sc)
    got = _feature_backward(sc, gpu, sc["dL"], fg.feature_rows(sc["base"], fg.ALL_C),
                            fg.feature_dL(sc["base"], fg.ALL_C), camera=True, antialiasing=True,
                            **{f"dL_d{n}": to_dev(dLp[i], gpu) for i, n in enumerate(pg.PLANES)})
    seen = _check("features", got, _reference("features", sc, gpu), sc, f"{sc['name']}/features")
    assert set(seen) == set(ps.POSE_F32_SPREAD["features"])


# ---- f --------------------------------------------------------------------------------------------
STRIPS = ((0, 1), (1, 2))


def _strip_call(sc, gpu, strip, det):
    s, d = sc["s"], _inputs(sc, gpu)
    y0, y1 = ss.pixel_rows(sc, strip)
    g = rasterize_gaussians_backward_native(
        to_dev(s["bg"], gpu), d["means3D"], d["colors_precomp"], d["opacities"], d["scales"],
        d["rotations"], s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], to_dev(sc["dL"][:, y0:y1], gpu), d["shs"],
        s["sh_degree"], to_dev(s["campos"], gpu), deterministic=det, tile_rows=strip,
        image_height=sc["H"])
    return _f64({k: v.cpu().numpy() for k, v in g.items()})


@pytest.mark.parametrize("det", (False, True), ids=("default", "deterministic"))
@pytest.mark.parametrize("pose", ps.NAMES)
def test_strips_add_up_to_the_frame(pose, det, gpu):
    """The strips' float64 references (the frame's with the image gradient zero outside the
    strip's rows) add up to the frame's exactly, so the strips' device gradients, added in float64,
    may differ from it by the sum of the strips' own allowances: bound x max|the strip's
    reference|, tensor by tensor."""
    sc = ps.get("chain", pose)
    assert ss.grid(sc) == (3, 2)
    fwd = _forward(sc, gpu)
    lists, radii = (fwd["ranges"], fwd["point_list"]), fwd["radii"]
    whole = _reference("colour", sc, gpu)
    total, allow, ref_sum = {}, {}, {}
    for strip in STRIPS:
        y0, y1 = ss.pixel_rows(sc, strip)
        dL = np.zeros_like(sc["dL"])
        dL[:, y0:y1] = sc["dL"][:, y0:y1]
        key = ("strip", sc["name"], strip)
        if key not in _ref_cache:
            _ref_cache[key] = gr.scene_gradients(sc, lists, radii, dL, gates=whole["gates"])
        ref = _ref_cache[key]
        got = _strip_call(sc, gpu, strip, det)
        for out, k in END_TO_END:
            if out in got and k in whole and np.abs(whole[k]).max() > 0:
                total[k] = total.get(k, 0.0) + got[out].reshape(whole[k].shape)
                ref_sum[k] = ref_sum.get(k, 0.0) + ref[k]
                allow[k] = allow.get(k, 0.0) + ps.bound("colour", k) * np.abs(ref[k]).max()
    assert len(total) >= 6
    for k, v in total.items():
        assert np.abs(ref_sum[k] - whole[k]).max() <= 1e-12 * np.abs(whole[k]).max(), k
        d = float(np.abs(v - whole[k]).max())
        worst[("strips", k)] = max(worst.get(("strips", k), 0.0), d / allow[k])
        print(f"{sc['name']}/strips/{det}: |sum - frame|[{k}] = {d:.3e} = {d / allow[k]:.3f} of "
              f"{allow[k]:.3e}")
        assert d <= allow[k], (k, d, allow[k])


# ---- g --------------------------------------------------------------------------------------------
def _quaternion(R):
    """(r, x, y, z) of a rotation matrix, float64."""
    r = 0.5 * np.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 0.0))
    assert r > 0.1
    return np.array([r, (R[2, 1] - R[1, 2]) / (4 * r), (R[0, 2] - R[2, 0]) / (4 * r),
                     (R[1, 0] - R[0, 1]) / (4 * r)])


def _view_of(q, t):
    """The (4, 4) GL view of a unit quaternion (r, x, y, z) and a translation, in q's dtype."""
    r, x, y, z = q[0], q[1], q[2], q[3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]).reshape(3, 3)
    last = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=q.dtype, device=q.device)
    return torch.cat([torch.cat([R, t.reshape(3, 1)], 1), last], 0)


def _unit(q):
    return q / q.norm()


def test_pose_leaf_through_the_rasterizer(gpu):
    """test_gpu_camera_gradients.test_pose_chain at the oblique pose, with the planes and a
    pose of seven parameters: q.grad and t.grad against the float64 reference's three partials at
    the camera the device read, pulled back through the chain's float64 Jacobian.  Entry j may
    differ by sum_k |Jac[k, j]| bound_k S_k -- each camera entry's own bound through the chain's
    linear map -- plus the float32 rounding of the chain's backward: 48 ulp of the term magnitudes
    |Jn|^T |JR|^T |J2|^T |g| (16 for camera_tensors' inverse and product, as test_pose_chain
    counts them; 24 for the rotation's nine entries, each q component gathering up to 18 terms; 8
    for the normalisation).  The Gaussians' own gradients: the planes' bound, every entry."""
    sc = ps.get("chain", "oblique")
    dLp = ps.plane_dL(sc)
    view_np, proj_gl = ps.gl_camera(sc["W"], sc["H"], "oblique")
    q0 = _quaternion(view_np[:3, :3].astype(np.float64)).astype(np.float32)
    t0 = np.ascontiguousarray(view_np[:3, 3], np.float32)
    assert np.abs(q0).min() > 0.05
    d = _inputs(sc, gpu)
    for v in d.values():
        if v is not None:
            v.requires_grad_(True)
    means2D = torch.zeros_like(d["means3D"], requires_grad=True)
    q = torch.tensor(q0, device=gpu, requires_grad=True)
    t = torch.tensor(t0, device=gpu, requires_grad=True)
    vm, pm, c = camera_tensors(_view_of(_unit(q), t), proj_gl)
    out = GaussianRasterizer(_settings(sc, gpu, vm, pm, c, depth_maps=True))(means2D=means2D, **d)
    assert len(out) == 5
    loss = (out[0] * to_dev(sc["dL"], gpu)).sum()
    for i in range(3):
        loss = loss + (out[2 + i] * to_dev(dLp[i], gpu)).sum()
    loss.backward()
    got = np.concatenate([q.grad.cpu().numpy(), t.grad.cpu().numpy()]).astype(np.float64)

    # the reference at the camera the device read (camera_tensors' float32 outputs)
    cam_np = [x.detach().cpu().numpy() for x in (vm, pm, c)]
    assert np.abs(cam_np[0] - sc["s"]["view"]).max() <= 1e-6  # the oblique pose, up to rounding
    leaves = tuple(torch.tensor(x.astype(np.float64).reshape(-1), requires_grad=True) for x in cam_np)
    res = run_hip(dict(sc["s"], view=cam_np[0], proj=cam_np[1], campos=cam_np[2]), gpu,
                  extras=ALL_EXTRAS, binning=True)
    ref = cg.scene_gradients(sc, (res["ranges"], res["point_list"]), res["radii"], sc["dL"], dLp,
                             camera=leaves)
    assert ref["near"] == (0, 0)
    g = np.concatenate([ref[n] for n in cg.CAMERA])
    jac = torch.autograd.functional.jacobian
    q64, t64 = torch.tensor(q0.astype(np.float64)), torch.tensor(t0.astype(np.float64))
    flat = lambda cam: torch.cat([x.reshape(-1) for x in cam])  # noqa: E731
    J = torch.cat(jac(lambda a, b: flat(camera_tensors(_view_of(_unit(a), b), proj_gl)),
                      (q64, t64)), 1).numpy()                                        # [35, 7]
    Jn = jac(_unit, q64).numpy()                                                     # [4, 4]
    JR = torch.cat(jac(lambda a, b: _view_of(a, b).reshape(-1), (_unit(q64), t64)), 1).numpy()
    J2 = jac(lambda v: flat(camera_tensors(v, proj_gl)),
             _view_of(_unit(q64), t64)).reshape(35, 16).numpy()
    stage0 = np.block([[Jn, np.zeros((4, 3))], [np.zeros((3, 4)), np.eye(3)]])
    assert np.abs(J2 @ JR @ stage0 - J).max() <= 1e-12 * np.abs(J).max()
    want = J.T @ g
    per_entry = np.concatenate([np.full(len(ref[n]), ps.bound("camera", n) * ref["S"][n])
                                for n in cg.CAMERA])
    m = np.abs(JR).T @ (np.abs(J2).T @ np.abs(g))
    m = np.concatenate([np.abs(Jn).T @ m[:4], m[4:]])
    tol = np.abs(J).T @ per_entry + 48 * 2.0 ** -23 * m
    ratio = np.abs(got - want) / tol
    worst[("pose leaf", "q, t")] = float(ratio.max())
    print(f"pose leaf: max|grad - ref| / tol = {ratio.max():.3f}, tol / max|ref| = "
          f"{(tol / np.abs(want).max()).round(7)}, ref = {want.round(4)}")
    assert (np.abs(got - want) <= tol).all(), (got - want, tol)
    assert (np.abs(want) > 0).all() and tol.max() <= 1e-2 * np.abs(want).max()
    grad = lambda x: x.grad.cpu().numpy()  # noqa: E731
    seen = _check("planes", dict(dL_dmeans3D=grad(d["means3D"]), dL_dmeans2D=grad(means2D),
                                 dL_dopacity=grad(d["opacities"]), dL_dscales=grad(d["scales"]),
                                 dL_drotations=grad(d["rotations"]), dL_dsh=grad(d["shs"])),
                  ref, sc, "pose leaf")
    assert len(seen) >= 6


def test_report_worst_ratio():
    """Not a check of its own: prints the largest e / bound the tests above saw per kind and
    tensor (DESIGN.md 4 quotes it)."""
    for (kind, key), v in sorted(worst.items()):
        print(f"worst {kind:9s} {key:11s} {v:.3f}")
    assert all(v <= 1.0 for v in worst.values())
