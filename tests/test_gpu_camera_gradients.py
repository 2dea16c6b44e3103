"""The gradients of the camera -- viewmatrix, projmatrix, campos (gsr_backward_camera, DESIGN.md
3h) -- on the device, against autograd of the float64 restatement (camera_grad_reference) on the
scenes of camera_grad_scenes.

Per camera tensor e = max|g_gpu - g_ref64| / S, S = max over its entries of sum_i |G_i| (G_i the
reference's per-Gaussian contributions), must stay within 8 x f, f the reference's own float32
spread in that measure (camera_grad_reference.F32_SPREAD, measured on the CPU).  The reference's
integer decisions (lists, radii) are the GPU forward's exported state; its float gates are
float64's, and no scene has a decision within rounding of a gate.

   1 end to end by ctypes: six scenes, the colour loss and colour + three planes; exact zeros
   2 the Gaussians' own gradients are untouched by the camera's
   3 through autograd, one camera tensor at a time, depth_maps False and True
   4 a pose leaf through camera.camera_tensors
   5 the translation identity among the call's own outputs
   6 the forward identities
   7 a NULL struct is gsr_backward_planes; one member alone
   8 degenerate frames: P == 0, everything culled
   9 statelessness, repeated calls
  10 errors
"""
import ctypes

import numpy as np
import pytest
import torch

import camera_grad_reference as cg
import camera_grad_scenes
import grad_reference as gr
import grad_scenes
import plane_grad_reference as pg
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.camera import camera_tensors, static_camera
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer,
                                                    rasterize_gaussians_backward_native)
from gpu_helpers import ALL_EXTRAS, run_hip, to_dev
from test_gpu_backward import END_TO_END, _forward, _inputs

pytestmark = pytest.mark.gpu

_ref_cache = {}
worst = {}  # the largest e / bound seen per camera tensor (printed by the last test)


def _loss_gradients(sc, loss):
    """(dL, dLp) of a loss of cg.LOSSES: the scene's image gradient, and with "combined" the three
    planes' gradients."""
    return sc["dL"], (camera_grad_scenes.plane_dL(sc["name"]) if loss == "combined" else None)


def _reference(sc, gpu, loss):
    key = (sc["name"], loss)
    if key not in _ref_cache:
        fwd = _forward(sc, gpu)
        ref = cg.scene_gradients(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"],
                                 *_loss_gradients(sc, loss))
        assert ref["near"] == (0, 0)
        _ref_cache[key] = ref
    return _ref_cache[key]


def _backward(sc, gpu, loss, camera=True):
    """gsr_backward_camera by ctypes under a loss of cg.LOSSES."""
    s, d = sc["s"], _inputs(sc, gpu)
    dL, dLp = _loss_gradients(sc, loss)
    planes = {} if dLp is None else {f"dL_d{n}": to_dev(dLp[i], gpu)
                                     for i, n in enumerate(pg.PLANES)}
    g = rasterize_gaussians_backward_native(
        to_dev(s["bg"], gpu), d["means3D"], d["colors_precomp"], d["opacities"], d["scales"],
        d["rotations"], s["scale_modifier"], d["cov3D_precomp"], to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], to_dev(dL, gpu), d["shs"], s["sh_degree"],
        to_dev(s["campos"], gpu), camera=camera, **planes)
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items()}


def _camera_close(got, ref, what, names=cg.CAMERA):
    """The failures of the camera tensors of `got` (by gsr_camera_gradients names or cg.CAMERA's)
    against a reference of cg.scene_gradients."""
    bad = []
    for n in names:
        v = got[n] if n in got else got["dL_d" + n]
        e, b = cg.cam_err(v, ref, n), cg.bound(n)
        worst[n] = max(worst.get(n, 0.0), e / b)
        print(f"{what}: e[{n}] = {e:.3e}  (bound {b:.1e}, S = {ref['S'][n]:.3e}, "
              f"max|ref| = {np.abs(ref[n]).max():.3e})")
        if not e <= b:
            bad.append(f"{what}: e[{n}] = {e:.3e} > {b:.1e}")
    return bad


def _never_read_are_zero(got, sc):
    vm, pm = got["dL_dviewmatrix"].reshape(-1), got["dL_dprojmatrix"].reshape(-1)
    assert (vm[3::4] == 0.0).all() and (pm[2::4] == 0.0).all()
    assert np.abs(vm).max() > 0 and np.abs(pm).max() > 0
    if sc["colors"] is not None:
        assert (got["dL_dcampos"] == 0.0).all()
    else:
        assert np.abs(got["dL_dcampos"]).max() > 0


@pytest.mark.parametrize("loss", cg.LOSSES)
@pytest.mark.parametrize("name", camera_grad_scenes.NAMES)
def test_end_to_end(name, loss, gpu):
    """Check 1: the three camera tensors by ctypes; the entries the forward never reads are 0.0."""
    sc = camera_grad_scenes.get(name)
    fwd = _forward(sc, gpu)
    if name == "sparse":  # the forward keeps chain's Gaussians and nothing else
        kept = np.flatnonzero(fwd["radii"] > 0)
        assert len(fwd["radii"]) == 66000 and set(kept) <= set(sc["special"]["kept"])
        assert len(kept) == int((_forward(grad_scenes.get("chain"), gpu)["radii"] > 0).sum())
    ref = _reference(sc, gpu, loss)
    got = _backward(sc, gpu, loss)
    assert got["dL_dviewmatrix"].shape == got["dL_dprojmatrix"].shape == (4, 4)
    assert got["dL_dcampos"].shape == (3,)
    bad = _camera_close(got, ref, f"{name}/{loss}")
    assert not bad, bad
    _never_read_are_zero(got, sc)


@pytest.mark.parametrize("loss", cg.LOSSES)
@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_other_gradients_untouched(name, loss, gpu):
    """Check 2: with the camera asked for, the Gaussians' gradients stay within the bounds of
    grad_reference (colour) and plane_grad_reference (combined) against those references."""
    sc = grad_scenes.get(name)
    fwd = _forward(sc, gpu)
    lists = (fwd["ranges"], fwd["point_list"])
    if loss == "colour":
        ref, bound = gr.scene_gradients(sc, lists, fwd["radii"], sc["dL"]), gr.bound
    else:
        ref = pg.scene_gradients(sc, lists, fwd["radii"], *pg.loss_gradients(sc, "combined"))
        bound = pg.bound
    got = _backward(sc, gpu, loss)
    bad = []
    for n, key in END_TO_END:
        if key in ref and n in got:
            e = gr.rel_err(got[n].reshape(ref[key].shape), ref[key])
            print(f"{name}/{loss}: e[{key}] = {e:.3e}  (bound {bound(key):.1e})")
            if not e <= bound(key):
                bad.append((key, e))
    assert not bad, bad
    assert (got["dL_dmeans3D"][fwd["radii"] == 0] == 0).all()


def _settings(sc, gpu, view, proj, campos, **kw):
    s = sc["s"]
    return GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"], view, proj,
        s["sh_degree"], campos, False, False, **kw)


def _loss_of(sc, gpu, loss):
    dL, dLp = _loss_gradients(sc, loss)

    def f(out):
        total = (out[0] * to_dev(dL, gpu)).sum()
        if dLp is not None:
            for i in range(3):
                total = total + (out[2 + i] * to_dev(dLp[i], gpu)).sum()
        return total
    return f


@pytest.mark.parametrize("depth_maps", (False, True))
@pytest.mark.parametrize("which", cg.CAMERA)
def test_through_autograd(which, depth_maps, gpu):
    """Check 3 (S1): GaussianRasterizer with one camera tensor requiring a gradient (the other two
    do not); the gradient has the input's shape, dtype and device."""
    sc = grad_scenes.get("chain")
    s, d = sc["s"], _inputs(sc, gpu)
    loss = "combined" if depth_maps else "colour"
    ref = _reference(sc, gpu, loss)
    cam = dict(viewmatrix=to_dev(s["view"], gpu), projmatrix=to_dev(s["proj"], gpu),
               campos=to_dev(s["campos"], gpu))
    cam[which].requires_grad_(True)
    rs = _settings(sc, gpu, cam["viewmatrix"], cam["projmatrix"], cam["campos"],
                   depth_maps=depth_maps)
    out = GaussianRasterizer(rs)(means2D=None, **d)
    assert len(out) == (5 if depth_maps else 2) and not out[1].requires_grad
    _loss_of(sc, gpu, loss)(out).backward()
    for n, t in cam.items():
        if n != which:
            assert t.grad is None
    g = cam[which].grad
    assert g.shape == cam[which].shape and g.dtype == torch.float32 and g.device == cam[which].device
    bad = _camera_close({which: g.cpu().numpy()}, ref, f"autograd/{which}/{depth_maps}", (which,))
    assert not bad, bad
    assert d["means3D"].grad is None


def _gl_camera(sc):
    cam = static_camera(sc["W"], sc["H"])
    return np.array(cam.get_view_matrix(), np.float32), cam.get_project_matrix()


@pytest.mark.parametrize("name", ("chain", "edges"))
def test_pose_chain(name, gpu):
    """Check 4: a (4, 4) GL view leaf through camera_tensors into the rasterizer and a linear
    loss; view.grad against the float64 reference chained through the same helper: the reference's
    three partials at the camera the device read, pulled back through camera_tensors' float64
    Jacobian.  Entry j of view.grad may differ by sum_k |Jac[k, j]| bound_k S_k -- each camera
    entry's own bound through the chain's linear map -- plus the float32 rounding of that map
    (16 ulp of sum_k |Jac[k, j]| |g_k|: the backward of the inverse and of proj @ view are two 4 x 4
    products each, every entry a 4-term sum).
    edges has clamped Gaussians: the cx dtxc term of dt.z is live."""
    sc = grad_scenes.get(name)
    d = _inputs(sc, gpu)
    view_np, proj_gl = _gl_camera(sc)
    view = torch.tensor(view_np, device=gpu, requires_grad=True)
    vm, pm, c = camera_tensors(view, proj_gl)
    out = GaussianRasterizer(_settings(sc, gpu, vm, pm, c))(means2D=None, **d)
    (out[0] * to_dev(sc["dL"], gpu)).sum().backward()
    assert view.grad is not None and tuple(view.grad.shape) == (4, 4)
    got = view.grad.cpu().numpy().astype(np.float64).reshape(-1)

    # the reference at the camera the device read (camera_tensors' float32 outputs)
    leaves = tuple(torch.tensor(t.detach().cpu().numpy().astype(np.float64).reshape(-1),
                                requires_grad=True) for t in (vm, pm, c))
    res = run_hip(dict(sc["s"], view=vm.detach().cpu().numpy(), proj=pm.detach().cpu().numpy(),
                       campos=c.detach().cpu().numpy()), gpu, colors_precomp=sc["colors"],
                  cov3D_precomp=sc["cov6"], extras=ALL_EXTRAS, binning=True)
    ref = cg.scene_gradients(sc, (res["ranges"], res["point_list"]), res["radii"], sc["dL"],
                             camera=leaves)
    assert ref["near"] == (0, 0)
    v64 = torch.tensor(view_np.astype(np.float64), requires_grad=True)
    jac = torch.autograd.functional.jacobian(
        lambda v: torch.cat([t.reshape(-1) for t in camera_tensors(v, proj_gl)]), v64)
    jac = jac.reshape(35, 16).numpy()
    g = np.concatenate([ref[n] for n in cg.CAMERA])
    want = jac.T @ g
    per_entry = np.concatenate([np.full(len(ref[n]), cg.bound(n) * ref["S"][n]) for n in cg.CAMERA])
    tol = np.abs(jac).T @ per_entry + 16 * 2.0 ** -23 * (np.abs(jac).T @ np.abs(g))
    print(f"{name}: max|view.grad - ref| / tol = {np.abs((got - want) / np.maximum(tol, 1e-300)).max():.3f}, "
          f"max|ref| = {np.abs(want).max():.3e}")
    assert (np.abs(got - want) <= tol).all(), (got - want, tol)
    assert np.abs(want).max() > 0


@pytest.mark.parametrize("name", ("chain", "sparse"))
def test_translation_identity(name, gpu):
    """Check 5: moving every Gaussian by dx is moving the camera the other way, so for c in 0..2
    sum_i dL_dmeans3D[i][c] = sum_r pm[4c+r] dL_dpm[12+r] + sum_r vm[4c+r] dL_dvm[12+r] -
    dL_dcampos[c], an exact relation among one call's outputs.  Both sides are sums of the same
    per-Gaussian terms, so they agree within the camera bound relative to sum_i
    |dL_dmeans3D[i][c]|."""
    sc = camera_grad_scenes.get(name)
    s = sc["s"]
    for loss in cg.LOSSES:
        got = _backward(sc, gpu, loss)
        vm = np.asarray(s["view"], np.float64).reshape(-1)
        pm = np.asarray(s["proj"], np.float64).reshape(-1)
        dvm, dpm = got["dL_dviewmatrix"].reshape(-1), got["dL_dprojmatrix"].reshape(-1)
        bnd = max(cg.bound(n) for n in cg.CAMERA)
        for c in range(3):
            lhs = got["dL_dmeans3D"][:, c].sum()
            rhs = (pm[4 * c:4 * c + 4] * dpm[12:16]).sum() + (vm[4 * c:4 * c + 4] * dvm[12:16]).sum() \
                - got["dL_dcampos"][c]
            scale = np.abs(got["dL_dmeans3D"][:, c]).sum()
            print(f"{name}/{loss}/{c}: lhs = {lhs:.6e}, rhs = {rhs:.6e}, "
                  f"|diff| / scale = {abs(lhs - rhs) / scale:.3e}  (bound {bnd:.1e})")
            assert abs(lhs - rhs) <= bnd * scale


@pytest.mark.parametrize("depth_maps", (False, True))
def test_forward_identities(depth_maps, gpu):
    """Check 6: with a camera tensor requiring a gradient the outputs are the bits of today's call;
    under no_grad nothing is saved and there is no graph."""
    sc = grad_scenes.get("chain")
    s, d = sc["s"], _inputs(sc, gpu)
    cam = [to_dev(s[k], gpu) for k in ("view", "proj", "campos")]
    plain = GaussianRasterizer(_settings(sc, gpu, *cam, depth_maps=depth_maps))(means2D=None, **d)
    assert all(t.grad_fn is None for t in plain)
    cam[0].requires_grad_(True)
    rs = _settings(sc, gpu, *cam, depth_maps=depth_maps)
    out = GaussianRasterizer(rs)(means2D=None, **d)
    assert len(out) == len(plain)
    assert [t.grad_fn is not None for t in out] == [i != 1 for i in range(len(out))]
    assert "Camera" in type(out[0].grad_fn).__name__
    for a, b in zip(out, plain):
        assert a.dtype == b.dtype and a.shape == b.shape
        np.testing.assert_array_equal(a.detach().cpu().numpy().view(np.uint32),
                                      b.cpu().numpy().view(np.uint32))
    with torch.no_grad():
        out = GaussianRasterizer(rs)(means2D=None, **d)
    assert all(t.grad_fn is None and not t.requires_grad for t in out)
    for a, b in zip(out, plain):
        np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32),
                                      b.cpu().numpy().view(np.uint32))


def _raw(sc, gpu, camera, dL=None, planes=None, strip=False, P=None, means3D=None):
    """gsr_backward_camera through the C ABI with the structs built here.  camera: a set of
    cg.CAMERA names to ask for, or None for a NULL struct.  Returns (rc, Gaussians' gradients,
    camera buffers); every buffer is pre-filled with 7.0."""
    s, d = sc["s"], _inputs(sc, gpu)
    if means3D is not None:
        d["means3D"] = means3D
    P = len(s["g"].xyz) if P is None else P
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
    n = max(P, 1)
    shapes = dict(dL_dmeans3D=(n, 3), dL_dmeans2D=(n, 3), dL_dopacity=(n, 1), dL_dcolors=(n, 3))
    if d["shs"] is not None:
        shapes["dL_dsh"] = (n, 16, 3)
    if d["scales"] is not None:
        shapes.update(dL_dscales=(n, 3), dL_drotations=(n, 4))
    grads = {k: torch.full(sh, 7.0, device=gpu) for k, sh in shapes.items()}
    out = _lib.GsrGradients(**{k: t.data_ptr() for k, t in grads.items()})
    bufs = {"viewmatrix": torch.full((16,), 7.0, device=gpu),
            "projmatrix": torch.full((16,), 7.0, device=gpu),
            "campos": torch.full((3,), 7.0, device=gpu)}
    cs = None if camera is None else _lib.GsrCameraGradients(
        **{"dL_d" + k: bufs[k].data_ptr() for k in camera})
    inp = _lib.GsrBackwardInputs(dL_dcolor=_lib.ptr(dL))
    rc = _lib.backward_camera_fn(_lib.load_library())(
        _lib.context(gpu.index or 0), ctypes.byref(g), ctypes.byref(st), ctypes.byref(inp),
        None if planes is None else ctypes.byref(planes), None if cs is None else ctypes.byref(cs),
        ctypes.byref(out), ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    torch.cuda.synchronize(gpu)
    return (rc, {k: v.cpu().numpy().astype(np.float64) for k, v in grads.items()},
            {k: v.cpu().numpy().astype(np.float64) for k, v in bufs.items()})


def test_null_struct_and_single_members(gpu):
    """Check 7: a NULL gsr_camera_gradients, and one with three NULL members, give
    gsr_backward_planes' results within its bounds and write no camera buffer; one member alone is
    within the camera bound, the other buffers untouched."""
    sc = grad_scenes.get("chain")
    fwd = _forward(sc, gpu)
    dL = to_dev(sc["dL"], gpu)
    dLp = [to_dev(p, gpu) for p in pg.plane_dL("chain")]
    planes = _lib.GsrPlaneGradients(dL_ddepth_map=dLp[0].data_ptr(),
                                    dL_dinv_depth_map=dLp[1].data_ptr(),
                                    dL_dfinal_T=dLp[2].data_ptr())
    ref = pg.scene_gradients(sc, (fwd["ranges"], fwd["point_list"]), fwd["radii"],
                             *pg.loss_gradients(sc, "combined"))
    for what, camera in (("NULL struct", None), ("three NULLs", ())):
        rc, got, bufs = _raw(sc, gpu, camera, dL, planes)
        assert rc == 0, what
        bad = []
        for n, key in END_TO_END:
            if key in ref and n in got:
                e = gr.rel_err(got[n].reshape(ref[key].shape), ref[key])
                print(f"{what}: e[{key}] = {e:.3e}  (bound {pg.bound(key):.1e})")
                if not e <= pg.bound(key):
                    bad.append((what, key, e))
        assert not bad, bad
        assert all((v == 7.0).all() for v in bufs.values())
    cref = _reference(sc, gpu, "combined")
    for one in cg.CAMERA:
        rc, _, bufs = _raw(sc, gpu, (one,), dL, planes)
        assert rc == 0
        bad = _camera_close(bufs, cref, f"{one} alone", (one,))
        assert not bad, bad
        assert all((v == 7.0).all() for k, v in bufs.items() if k != one)


def test_one_member_has_the_bits_of_all_three(gpu):
    """Check 7, the bits: the per-Gaussian stage and the finish are functions of the 2D gradient
    rows, and a row is reproducible when one wave alone adds to it.  So: one Gaussian (P = 1) of
    chain, shrunk until its 2D covariance is the 0.3 low-pass (alpha < 1 / 255 from 3 px on), whose
    centre lies 3 px or more inside one 8 x 8 quadrant -- only that quadrant's wave contributes.
    Then a member alone has the bits it has when all three are asked for."""
    sc = grad_scenes.get("chain")
    dL = to_dev(sc["dL"], gpu)
    fwd = _forward(sc, gpu)
    m = np.mod(fwd["means2D"], 8.0)
    inside = (fwd["radii"] > 0) & (m >= 2.0).all(1) & (m <= 5.0).all(1) & \
        (fwd["means2D"] >= 0).all(1) & (fwd["means2D"][:, 0] <= sc["W"] - 1) & \
        (fwd["means2D"][:, 1] <= sc["H"] - 1)
    assert inside.any()
    i = int(np.flatnonzero(inside)[0])
    one = {k: (None if v is None else v[i:i + 1].contiguous()) for k, v in _inputs(sc, gpu).items()}
    one["scales"] = torch.full((1, 3), 0.001, device=gpu)
    s = sc["s"]

    def call(names):
        keep = [to_dev(s[k], gpu) for k in ("view", "proj", "campos", "bg")]
        g = _lib.GsrGaussians(P=1, D=s["sh_degree"], M=16, scale_modifier=s["scale_modifier"],
                              means3D=_lib.ptr(one["means3D"]), scales=_lib.ptr(one["scales"]),
                              rotations=_lib.ptr(one["rotations"]),
                              opacities=_lib.ptr(one["opacities"]), shs=_lib.ptr(one["shs"]))
        st = _lib.GsrRasterSettings(image_width=sc["W"], image_height=sc["H"], tanfovx=s["tx"],
                                    tanfovy=s["ty"], viewmatrix=_lib.ptr(keep[0]),
                                    projmatrix=_lib.ptr(keep[1]), campos=_lib.ptr(keep[2]),
                                    bg=_lib.ptr(keep[3]))
        bufs = {"viewmatrix": torch.full((16,), 7.0, device=gpu),
                "projmatrix": torch.full((16,), 7.0, device=gpu),
                "campos": torch.full((3,), 7.0, device=gpu)}
        cs = _lib.GsrCameraGradients(**{"dL_d" + k: bufs[k].data_ptr() for k in names})
        m3 = torch.zeros((1, 3), device=gpu)
        rc = _lib.backward_camera_fn(_lib.load_library())(
            _lib.context(gpu.index or 0), ctypes.byref(g), ctypes.byref(st),
            ctypes.byref(_lib.GsrBackwardInputs(dL_dcolor=dL.data_ptr())), None, ctypes.byref(cs),
            ctypes.byref(_lib.GsrGradients(dL_dmeans3D=m3.data_ptr())),
            ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
        torch.cuda.synchronize(gpu)
        assert rc == 0
        return {k: v.cpu().numpy() for k, v in bufs.items()}, m3.cpu().numpy()
    all3, m3_all = call(cg.CAMERA)
    assert all(np.abs(v).max() > 0 for v in all3.values()) and np.abs(m3_all).max() > 0
    for n in cg.CAMERA:
        alone, m3 = call((n,))
        np.testing.assert_array_equal(m3.view(np.uint32), m3_all.view(np.uint32))
        np.testing.assert_array_equal(alone[n].view(np.uint32), all3[n].view(np.uint32), n)
        assert all((v == 7.0).all() for k, v in alone.items() if k != n)


def test_degenerate_frames(gpu):
    """Check 8: P == 0, and a frame where everything is culled (every Gaussian behind the eye):
    the camera buffers, pre-filled with 7.0, come back exactly 0.0 and rc == 0."""
    sc = grad_scenes.get("chain")
    dL = to_dev(sc["dL"], gpu)
    rc, _, bufs = _raw(sc, gpu, cg.CAMERA, dL, P=0)
    assert rc == 0
    assert all((v == 0.0).all() for v in bufs.values()), bufs
    behind = to_dev(sc["s"]["g"].xyz, gpu).clone()
    behind[:, 2] += 6.0  # the eye is at z = 4 looking down -z
    rc, got, bufs = _raw(sc, gpu, cg.CAMERA, dL, means3D=behind.contiguous())
    assert rc == 0
    assert all((v == 0.0).all() for v in bufs.values()), bufs
    assert all((v == 0.0).all() for v in got.values())


def test_statelessness_and_repeats(gpu):
    """Check 9: backward A, forward B, backward A again, and B twice, all within the bounds (two
    calls on identical 2D gradient rows cannot be arranged from outside: the rows come from float
    atomics; DESIGN.md 3h states the finish's bit-reproducibility)."""
    a, b = grad_scenes.get("chain"), camera_grad_scenes.get("blocks")
    ref_a, ref_b = _reference(a, gpu, "combined"), _reference(b, gpu, "combined")
    bad = _camera_close(_backward(a, gpu, "combined"), ref_a, "A")
    _forward(b, gpu, cache=False)
    bad += _camera_close(_backward(a, gpu, "combined"), ref_a, "A after forward B")
    bad += _camera_close(_backward(b, gpu, "combined"), ref_b, "B after backward A")
    bad += _camera_close(_backward(b, gpu, "combined"), ref_b, "B again")
    bad += _camera_close(_backward(a, gpu, "colour"), _reference(a, gpu, "colour"), "A, colour")
    assert not bad, bad


def test_errors(gpu):
    """Check 10: a strip gives GSR_E_INVALID and nothing is written; a shading with a camera
    gradient raises in backward."""
    sc = grad_scenes.get("chain")
    lib = _lib.load_library()
    dL = to_dev(sc["dL"], gpu)
    rc, got, bufs = _raw(sc, gpu, cg.CAMERA, dL, strip=True)
    assert rc == -1 and b"gsr_backward_camera: whole frames only" in lib.gsr_last_error()
    assert all((v == 7.0).all() for v in got.values())
    assert all((v == 7.0).all() for v in bufs.values())
    s, d = sc["s"], _inputs(sc, gpu)
    view = to_dev(s["view"], gpu).requires_grad_(True)
    rs = _settings(sc, gpu, view, to_dev(s["proj"], gpu), to_dev(s["campos"], gpu),
                   shading=_lib.GSR_SHADE_FLAT_BALL)
    color, _ = GaussianRasterizer(rs)(means2D=None, **d)
    assert color.requires_grad
    with pytest.raises(RuntimeError, match="splat composite only"):
        color.sum().backward()
    assert view.grad is None


def test_report_worst_ratio():
    """Not a check of its own: prints the largest e / bound the tests above saw per camera tensor
    (DESIGN.md 3h quotes it)."""
    print({k: f"{v:.3f}" for k, v in worst.items()})
