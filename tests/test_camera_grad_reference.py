"""CPU: pins the reference of the camera-gradient tests (camera_grad_reference): its per-Gaussian
stage is grad_reference.project's, its camera gradients match central differences of its own
float64 loss, no scene has a decision within rounding of a gate, and the float32 spread the GPU
tolerance is built from is re-measured.  Also camera.camera_tensors against cuda_camera_inputs, and
the host side of gsr_backward_camera: exported, its struct laid out as the header's."""
import ctypes

import numpy as np
import pytest
import torch

import camera_grad_reference as cg
import camera_grad_scenes
import grad_reference as gr
import grad_scenes
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.camera import (camera_tensors, cuda_camera_inputs, orbit_eye,
                                                static_camera)
from test_grad_reference import _oracle

_ref_cache = {}


def _loss_gradients(sc, loss):
    """(dL, dLp) of a loss of cg.LOSSES."""
    return sc["dL"], (camera_grad_scenes.plane_dL(sc["name"]) if loss == "combined" else None)


def _ref64(sc, loss):
    key = (sc["name"], loss)
    if key not in _ref_cache:
        orc = _oracle(sc)
        _ref_cache[key] = cg.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"],
                                             *_loss_gradients(sc, loss))
    return _ref_cache[key]


def test_scene_shapes():
    """blocks: three blocks of 256, the last with 88 Gaussians, most of them kept.  sparse: 258
    blocks; the forward keeps chain's 96 Gaussians and nothing else, with chain's lists."""
    b = camera_grad_scenes.get("blocks")
    kept = _oracle(b)["radii"] > 0
    assert len(kept) == 600 and (600 + 255) // 256 == 3 and 600 - 512 == 88
    assert kept[:256].sum() > 128 and kept[256:512].sum() > 128 and kept[512:].sum() > 44
    s, chain = camera_grad_scenes.get("sparse"), grad_scenes.get("chain")
    orc, orc_c = _oracle(s), _oracle(chain)
    at = s["special"]["kept"]
    assert len(orc["radii"]) == 66000 and (66000 + 255) // 256 == 258 > 256
    np.testing.assert_array_equal(np.flatnonzero(orc["radii"] > 0), at[orc_c["radii"] > 0])
    np.testing.assert_array_equal(orc["ranges"], orc_c["ranges"])
    np.testing.assert_array_equal(orc["point_list"], at[orc_c["point_list"]])


@pytest.mark.parametrize("name", camera_grad_scenes.NAMES)
def test_project_is_grad_reference_project(name):
    """The restated per-Gaussian stage equals gr.project in float64: means2D_px, conic and rgb to
    1e-14 relative, and its z is plane_grad_reference's."""
    import plane_grad_reference as pg
    sc = camera_grad_scenes.get(name)
    orc = _oracle(sc)
    lv = gr.leaves(sc, torch.float64)
    P = len(orc["radii"])
    cam = gr.camera_constants(sc["s"])
    args = (lv["means3D"], lv["means2D"], lv.get("scales"), lv.get("rotations"), lv.get("cov3D"),
            lv.get("shs"), lv.get("colors"))
    with torch.no_grad():
        want = gr.project(cam, orc["radii"], *args)
        vmP, pmP, cP = (t.reshape(1, -1).expand(P, -1)
                        for t in cg.camera_of(sc["s"], requires_grad=False))
        got = cg.project(cam, orc["radii"], vmP, pmP, cP, *args)
        z = pg.view_depth(cam, orc["radii"], lv["means3D"])
    for w, g, what in zip(want[:3], got[:3], ("means2D_px", "conic", "rgb")):
        assert gr.rel_err(g.numpy(), w.numpy()) <= 1e-14, what
    assert gr.rel_err(got[3].numpy(), z.numpy()) <= 1e-14
    assert got[5] == want[4]  # the same near-gate count


@pytest.mark.parametrize("loss", cg.LOSSES)
@pytest.mark.parametrize("name", camera_grad_scenes.NAMES)
def test_no_decision_near_its_gate(name, loss):
    ref = _ref64(camera_grad_scenes.get(name), loss)
    assert ref["near"] == (0, 0)
    assert ref["S"]["viewmatrix"] > 0 and ref["S"]["projmatrix"] > 0
    assert (ref["S"]["campos"] > 0) == (name != "precomputed")
    # entries the forward never reads
    assert (ref["viewmatrix"][3::4] == 0).all() and (ref["projmatrix"][2::4] == 0).all()


@pytest.mark.parametrize("loss", cg.LOSSES)
@pytest.mark.parametrize("name", camera_grad_scenes.NAMES)
def test_gradients_match_central_differences(name, loss):
    """Along random directions d in (vm, pm, c) space: (L(x + h d) - L(x - h d)) / 2h, h = 1e-6,
    against g . d, within 1e-6 of sum |g_k d_k| (the size of the terms of that dot product: float64
    central differences of these O(1) - O(100) losses give ~1e-9 of it).  The gates are the base
    run's, as the derivative holds them."""
    sc = camera_grad_scenes.get(name)
    orc = _oracle(sc)
    lists = (orc["ranges"], orc["point_list"])
    dL, dLp = _loss_gradients(sc, loss)
    ref = _ref64(sc, loss)
    g = np.concatenate([ref[n] for n in cg.CAMERA])
    x0 = np.concatenate([t.detach().numpy() for t in cg.camera_of(sc["s"])])
    lv = {k: v.detach() for k, v in gr.leaves(sc, torch.float64).items()}

    def L(x):
        cam = tuple(torch.tensor(v) for v in (x[:16], x[16:32], x[32:]))
        with torch.no_grad():
            return float(cg.scene_loss(sc, lists, orc["radii"], dL, dLp, cam, lv, ref["gates"])[0])
    assert abs(L(x0) - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
    rng = np.random.default_rng(5)
    h = 1e-6
    for _ in range(3):
        d = rng.standard_normal(35)
        fd = (L(x0 + h * d) - L(x0 - h * d)) / (2 * h)
        scale = np.abs(g * d).sum()
        print(f"{name}/{loss}: fd = {fd:.9e}, g.d = {g @ d:.9e}, sum|g d| = {scale:.3e}")
        assert abs(fd - g @ d) <= 1e-6 * scale


def test_float32_spread_constants():
    """cg.F32_SPREAD (the GPU tests' yardstick) is what a float32 evaluation of the reference gives
    here, to within a factor 2 either way."""
    seen, table = {}, {}
    for name in camera_grad_scenes.NAMES:
        sc = camera_grad_scenes.get(name)
        orc = _oracle(sc)
        for loss in cg.LOSSES:
            r64 = _ref64(sc, loss)
            r32 = cg.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"],
                                     *_loss_gradients(sc, loss), torch.float32, r64["gates"])
            for k in cg.CAMERA:
                if r64["S"][k] > 0:
                    e = cg.cam_err(r32[k], r64, k)
                    table[(name, loss, k)] = e
                    seen[k] = max(seen.get(k, 0.0), e)
    for k, e in table.items():
        print(k, f"{e:.2e}")
    print({k: f"{v:.3e}" for k, v in seen.items()})
    assert set(seen) == set(cg.F32_SPREAD)
    for k, f in seen.items():
        assert 0.5 * f <= cg.F32_SPREAD[k] <= 2.0 * f, (k, f, cg.F32_SPREAD[k])


def _gl_camera(cam):
    return np.array(cam.get_view_matrix(), np.float32), cam.get_project_matrix()


@pytest.mark.parametrize("eye", ((0.0, 0.0, 4.0), orbit_eye(137), orbit_eye(612)))
def test_camera_tensors_is_cuda_camera_inputs(eye):
    """camera_tensors reproduces cuda_camera_inputs: the view exactly (a sign), the projection to
    float32 rounding of a 4-term product sum (4 ulp of the largest entry), campos -- the inverse's
    translation against Camera.position -- to float32 rounding of the inverse."""
    cam = static_camera(40, 24, eye)
    view, proj = _gl_camera(cam)
    vm, pm, campos, _, _ = cuda_camera_inputs(cam)
    got = camera_tensors(torch.tensor(view), proj)
    assert got[0].dtype == torch.float32 and tuple(got[0].shape) == tuple(got[1].shape) == (4, 4)
    np.testing.assert_array_equal(got[0].numpy(), vm)
    ulp = 2.0 ** -23
    assert np.abs(got[1].numpy() - pm).max() <= 4 * ulp * np.abs(pm).max()
    assert np.abs(got[2].numpy() - campos).max() <= 8 * ulp * np.abs(campos).max()


def test_camera_tensors_is_differentiable():
    """The three outputs carry a graph to the view leaf; the gradient is gradcheck's."""
    cam = static_camera(40, 24, orbit_eye(137))
    view, proj = _gl_camera(cam)
    v = torch.tensor(view.astype(np.float64), requires_grad=True)
    out = camera_tensors(v, proj)
    assert all(t.requires_grad and t.dtype == torch.float64 for t in out)
    assert torch.autograd.gradcheck(lambda x: camera_tensors(x, proj), (v,), eps=1e-6, atol=1e-7)


def test_host_side_of_gsr_backward_camera():
    """The symbol is exported and declared; gsr_camera_gradients is three pointers."""
    assert "gsr_backward_camera" in _lib.EXPORTED_SYMBOLS
    assert ctypes.sizeof(_lib.GsrCameraGradients) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in _lib.GsrCameraGradients._fields_] == list(_lib.CAMERA_GRADIENT_NAMES)
    lib = _lib.load_library()
    assert _lib.backward_camera_fn(lib) is lib.gsr_backward_camera
    # argument validation needs no device
    rc = lib.gsr_backward_camera(None, None, None, None, None, None, None, None)
    assert rc == -1 and b"gsr_backward_camera: NULL argument" in lib.gsr_last_error()
